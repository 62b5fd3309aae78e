"""The op layer's launches, record by record, against the transcripts kept in tests/golden/op_launch_transcripts.json.

tests/launch_transcript.py replaces the library by a recorder and runs the op layer on CPU tensors: all twelve modes through
_Geo.fwd_desc, the eight trainable modes through conv_forward / conv_dgrad / conv_wgrad, the five block Functions forward and
backward (caches, in-place accumulation, deferred chain rule, the two-source GEMM's fallbacks, frozen weights) and the batch
chunking of launches.  Entry names, every integer / float argument, every descriptor field and which operand of the case a
pointer addresses (with its byte offset) must all be what the golden holds; pointers into temporaries are not compared (the
GPU test test_launches_in_batch_chunks_equal_one_launch holds the chunk offsets of outputs)."""
import json
import os

import pytest

import launch_transcript as LT

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "op_launch_transcripts.json")) as _f:
    GOLDEN = json.load(_f)


def test_golden_holds_exactly_the_cases():
    assert sorted(GOLDEN) == sorted(LT.CASES)


@pytest.mark.parametrize("name", list(LT.CASES))
def test_launch_transcript(name, monkeypatch):
    got = json.loads(json.dumps(LT.run_case(name, monkeypatch)))
    want = GOLDEN[name]
    assert got["acc_stats"] == want["acc_stats"] and got["in_place_params"] == want["in_place_params"]
    for i, (g, w) in enumerate(zip(got["records"], want["records"])):
        assert g == w, f"{name}: record {i} differs"
    assert len(got["records"]) == len(want["records"])
