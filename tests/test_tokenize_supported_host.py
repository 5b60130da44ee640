"""Which shapes the fused tokenize launch takes (``ops.tokenize_supported`` / ``ops.tokenize_fast_supported``), pinned on the host.

Both queries are pure host code: they size the workgroup's LDS (weights, biases, centring vector, stage ring: ``FusedLds``,
``csrc/lipvq_fused_lds.h``) and compare it with the 160 KiB a workgroup can have.  The kernel takes its LDS pointers from the same
description, and its device code is pinned by comparing assembly (``scripts/dev/asm_diff.sh``); this test pins the host half.

``tests/golden/tokenize_supported.json`` holds the answers over the grid below as recorded from the commit BEFORE the layout was
gathered into ``FusedLds`` (three free functions then sized the launch): one string of ``0``/``1`` over ``A`` per
``(J0, J1, D, K, query)``.  To record from another checkout (its library: ``LIPVQ_HIP_LIBRARY``, see ``_capi.py``):

    LIPVQ_HIP_LIBRARY=<a build of that checkout's csrc> python tests/test_tokenize_supported_host.py [out.json]
"""
import json
import sys
from pathlib import Path

import pytest

GOLDEN = Path(__file__).resolve().parent / "golden" / "tokenize_supported.json"

FAN_INS = tuple(range(66))                                   # 0 .. 65: both sides of the widest fan-in, 64
HIDDEN = ((64, 128), (128, 64), (64, 64))                    # the encoder's widths, and two stacks without an instance
WIDTHS = (16, 32, 48, 64, 128, 208)                          # the four latent widths with an instance, and two without
CODES = (0, 1, 2049)                                         # no codebook, the smallest, one past the LDS histogram's 2048
QUERIES = ("tokenize_supported", "tokenize_fast_supported")


def _key(J0, J1, D, K, query):
    return f"J0={J0}/J1={J1}/D={D}/K={K}/{query}"


def record(ops):
    """{row key: answers over FAN_INS as a string of 0/1}"""
    return {_key(J0, J1, D, K, q): "".join(str(int(getattr(ops, q)(A, J0, J1, D, K))) for A in FAN_INS)
            for J0, J1 in HIDDEN for D in WIDTHS for K in CODES for q in QUERIES}


def _ops():
    from lipvq_vae_amd import ops
    return ops


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())["rows"]


def test_grid_is_the_recorded_grid(golden):
    assert sorted(golden) == sorted(_key(J0, J1, D, K, q) for J0, J1 in HIDDEN for D in WIDTHS for K in CODES for q in QUERIES)
    assert all(len(v) == len(FAN_INS) and set(v) <= {"0", "1"} for v in golden.values())
    # the fixture is not vacuous: some shapes are taken, some refused, and D = 128 stops fitting at a fan-in inside the grid
    assert golden[_key(64, 128, 64, 1, "tokenize_supported")] == "0" + "1" * 64 + "0"
    row = golden[_key(64, 128, 128, 1, "tokenize_supported")]
    assert row[1] == "1" and row[64] == "0"


@pytest.mark.parametrize("query", QUERIES)
def test_answers_equal_the_recorded_ones(query, golden):
    got = record(_ops())
    for key in sorted(golden):
        if key.endswith("/" + query):
            assert got[key] == golden[key], f"{key}: answers over A = 0 .. 65 differ from the recorded ones"


if __name__ == "__main__":
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else GOLDEN
    rows = record(_ops())
    out.write_text(json.dumps({"recorded_from": "the commit before FusedLds", "rows": rows}, indent=0, separators=(",", ":")) + "\n")
    print(f"{len(rows)} rows of {len(FAN_INS)} answers -> {out}")
