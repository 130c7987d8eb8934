#!/usr/bin/env python
"""Golden table of the reference's shard wire format: every message / field / number / type / label and every rpc of the
reference's proto/generate.proto, as JSON.  The output (tests/golden/generate_proto_schema.json) is committed, this
script is how it was made; tests/test_pb_contract.py compares generate_pb2's descriptor table with it.

    python tests/golden/make_proto_schema.py <reference checkout>/proto/generate.proto"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def parse_proto(text):
    """{message: [(field, number, type, label)]}, {rpc: (request, response)} of a proto3 file (services skipped for fields)."""
    text = re.sub(r"//.*", "", text)
    toks = re.findall(r"[A-Za-z_][A-Za-z_0-9.]*|\d+|[{}=;()]", text)
    ref = {}
    stack = []
    i = 0
    while i < len(toks):
        t = toks[i]
        if t in ("message", "enum") and toks[i + 2] == "{":
            stack.append((t, ".".join([s[1] for s in stack if s[0] == "message"] + [toks[i + 1]])
                          if t == "message" else toks[i + 1]))
            if t == "message":
                ref.setdefault(stack[-1][1], [])
            i += 3
            continue
        if t == "service":
            depth = 0
            while True:  # skip the service block
                if toks[i] == "{":
                    depth += 1
                if toks[i] == "}":
                    depth -= 1
                    if depth == 0:
                        break
                i += 1
            i += 1
            continue
        if t == "}":
            stack.pop()
            i += 1
            continue
        if stack and stack[-1][0] == "message" and t not in ("message", "enum", "{", ";"):
            label = ""
            if t in ("repeated", "optional"):
                label = t
                i += 1
            ftype, fname, _eq, num = toks[i], toks[i + 1], toks[i + 2], toks[i + 3]
            ref[stack[-1][1]].append((fname, int(num), ftype.split(".")[-1], label))
            i += 5
            continue
        i += 1
    rpcs = {r[0]: (r[1], r[2]) for r in re.findall(r"rpc\s+(\w+)\s*\((\w+)\)\s*returns\s*\((\w+)\)", text)}
    return ref, rpcs


def main():
    messages, rpcs = parse_proto(open(sys.argv[1]).read())
    out = {"messages": {m: [list(f) for f in sorted(fs)] for m, fs in sorted(messages.items())},
           "rpcs": {r: list(io) for r, io in sorted(rpcs.items())}}
    with open(os.path.join(HERE, "generate_proto_schema.json"), "w") as f:  # one message / rpc per line
        f.write("{\"messages\": {\n")
        f.write(",\n".join(f" {json.dumps(m)}: {json.dumps(fs)}" for m, fs in out["messages"].items()))
        f.write("},\n\"rpcs\": {\n")
        f.write(",\n".join(f" {json.dumps(r)}: {json.dumps(io)}" for r, io in out["rpcs"].items()))
        f.write("}}\n")


if __name__ == "__main__":
    main()
