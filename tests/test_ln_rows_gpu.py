"""The output bits of the fp16 row-LayerNorm entry points are pinned: SHA-256 digests of every output buffer of
isic_layernorm_f16, isic_row_stats_f16, isic_layernorm_mxfp8_f16, isic_layernorm_add_f16, isic_layernorm_act_mxfp8_f16,
isic_layernorm_add_bwd_f16 and, for the MXFP8 tail they share, isic_mxfp8_quantize and isic_dwconv5x5_mxfp8_f16, on
the fixed inputs of tests/ln_rows_cases.py, against tests/golden/ln_rows_bits.json.

The golden file was written by tools/gen_ln_rows_bits.py on the MI355X from the commit BEFORE these kernels were moved
onto csrc/ln_rows.inc (every case ran twice there; all 412 digests were reproducible).  The five kernels share one
source text but the compiler contracts multiply-adds per kernel, so their statistics may differ from each other in the
last bit; this test pins each kernel's own bits.  The comparison is exact: a differing digest
means a change moved output bits, which is a change of behaviour and needs the golden file regenerated on purpose."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-isic_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ln_rows_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """a device error (not a failed comparison) ends the session: nothing more is launched on a GPU that has faulted"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error, no further GPU work: {e}", returncode=3)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "ln_rows_bits.json")) as f:
        doc = json.load(f)
    assert doc["not_reproducible"] == []
    return doc["digests"]


@pytest.mark.parametrize("group", sorted(C.GROUPS))
def test_layernorm_output_bits_are_the_pinned_ones(group, golden):
    got = C.digests(group)
    prefixes = {k.split("/")[0] for k in got}
    want = {k: v for k, v in golden.items() if k.split("/")[0] in prefixes}
    assert got.keys() == want.keys(), sorted(set(got) ^ set(want))
    differing = sorted(k for k in got if got[k] != want[k])
    assert not differing, f"{len(differing)} of {len(got)} buffers changed bits: {differing[:12]}"


def test_every_pinned_buffer_belongs_to_a_group(golden):
    entries = {k.split("/")[0] for k in golden}
    assert entries == {"isic_layernorm_f16", "isic_row_stats_f16", "isic_layernorm_mxfp8_f16", "isic_layernorm_add_f16",
                       "isic_layernorm_act_mxfp8_f16", "isic_layernorm_add_bwd_f16", "isic_mxfp8_quantize",
                       "isic_dwconv5x5_mxfp8_f16"}
