"""CPU: the protoc-free generate_pb2 speaks the reference's wire format (proto/generate.proto)."""
import json
import os

from tgis_amd.pb import generate_pb2 as pb

SCHEMA_FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "generate_proto_schema.json")


def test_roundtrip_and_presence():
    r = pb.Request(id=3, inputs="hi", input_length=2, max_output_length=5, truncate=True)
    r.parameters.seed = 7
    r.parameters.length_penalty.start_index = 4
    r.details.logprobs = True
    b = pb.Batch(id=1, requests=[r], total_tokens=2)
    b2 = pb.Batch.FromString(b.SerializeToString())
    assert b2.requests[0].parameters.HasField("seed") and b2.requests[0].parameters.seed == 7
    assert not b2.requests[0].parameters.HasField("repetition_penalty")
    assert b2.requests[0].parameters.HasField("length_penalty")
    assert not pb.NextTokenResponse().HasField("result")
    assert not pb.CachedBatch(batch_id=1).HasField("status")
    cb = pb.CachedBatch(batch_id=1)
    cb.status.completed_ids.extend([1, 5])
    assert pb.CachedBatch.FromString(cb.SerializeToString()).status.completed_ids == [1, 5]
    # hand-checked wire bytes: field 100 (min_new_tokens) varint tag = (100<<3)|0 = 800 -> 0xa0 0x06
    assert pb.NextTokenChooserParameters(min_new_tokens=3).SerializeToString() == b"\xa0\x06\x03"
    # healthcheck batch id 2**64-1 must be representable (server.py:37)
    assert pb.Batch.FromString(pb.Batch(id=2**64 - 1).SerializeToString()).id == 2**64 - 1


def test_field_numbers_match_reference_proto():
    """Every message/field/number/label and every rpc of the reference .proto equals our descriptor table
    (tests/golden/generate_proto_schema.json: the reference's proto/generate.proto as tests/golden/make_proto_schema.py
    parses it)."""
    ref = json.load(open(SCHEMA_FIXTURE))
    assert set(ref["messages"]) == set(pb.SCHEMA), set(ref["messages"]) ^ set(pb.SCHEMA)
    for msg, fields in ref["messages"].items():
        ours = {(n, num, t.split(":")[-1].split(".")[-1], lab) for n, num, t, lab in pb.SCHEMA[msg]}
        assert ours == {tuple(f) for f in fields}, (msg, ours ^ {tuple(f) for f in fields})
    assert {r: tuple(io) for r, io in ref["rpcs"].items()} == pb.RPCS
