// Host-side dispatch: a runtime value -> a tag whose type carries it, handed to a generic lambda that names the
// kernel instance.  Every f returns a TGIS_* code, which the helper passes on.  Only the listed values instantiate
// f; where not every combination has a kernel, the lambda guards with `if constexpr` (never a cartesian product) or lists
// the pairs that exist (by_pair).
#pragma once
#include <type_traits>
#include "common.h"

template <typename T> struct type_c { using type = T; };
template <typename Tag> using type_of = typename Tag::type;  // using T = type_of<decltype(t)>;
template <int V> using int_c = std::integral_constant<int, V>;  // constexpr int NT = decltype(nt)::value;

template <typename F> int by_dtype(int dtype, F&& f) { return dtype == TGIS_F16 ? f(type_c<f16>{}) : f(type_c<bf16>{}); }

// element of the KV pools: the model dtype T, or one-byte e4m3 codes (kv_layout.h)
template <typename T, typename F> int by_kv(bool kv8, F&& f) { return kv8 ? f(type_c<uint8_t>{}) : f(type_c<T>{}); }

template <typename F> int by_bool(bool b, F&& f) { return b ? f(std::true_type{}) : f(std::false_type{}); }

// (a, b) among the listed pairs only; in f: decltype(p)::first, decltype(p)::second
template <int A, int B> struct pair_c { static constexpr int first = A, second = B; };
template <typename... Ps, typename F> int by_pair(int a, int b, const char* what, F&& f) {
    int rc = TGIS_EINVAL;
    if (!((a == Ps::first && b == Ps::second && (rc = f(Ps{}), true)) || ...))
        tgis_set_error("%s: no kernel for (%d, %d)", what, a, b);
    return rc;
}

template <int... Vs, typename F> int by_int(int v, const char* what, F&& f) {
    int rc = TGIS_EINVAL;
    if (!((v == Vs && (rc = f(int_c<Vs>{}), true)) || ...)) tgis_set_error("%s: no kernel for %d", what, v);
    return rc;
}
