"""The tile sweeps of the wave-autonomous loop kernel after their non-product work moved between the matrix-core products, read from
the cross-compiled listing of the benchmark's dimension set (no GPU; built the way tests/test_wv_isa.py builds it) and set against the
parent's listing (profiles/wv_sweep_gaps_isa_before.json, tools/isa_loops.py): in each of the four sweep loops fewer products are
followed at once by another product, and neither the s_nop count nor the instruction count per trip went up.  No private segment."""
import importlib.util
import json
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSTR_DIMS = (3, 2, 3, 3, 3, 0, 0)
KERNEL = "loop_kernel_wvILi3ELi2ELi3ELi3ELi3ELb0ELi0ELi5ELb0ELi4E"
PARENT_INSTRS = (315, 70, 100, 70)      # tile_factor, tile_forward (predictor), tile_rhs, tile_forward (corrector), per trip of four blocks


def _isa_loops():
    spec = importlib.util.spec_from_file_location("isa_loops", os.path.join(ROOT, "tools", "isa_loops.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def listing(pkg, tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc: the listing cannot be made")
    from mpc_code_amd import capi
    out = str(tmp_path_factory.mktemp("wv_sweep_gaps") / "mpc_amd_cstr.s")
    flags = [f for f in capi.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    flags.append("-DMPC_DIM_LIST(X)=X(" + ",".join(str(v) for v in CSTR_DIMS) + ")")
    subprocess.check_call([HIPCC] + flags + ["--offload-device-only", "-S", "-o", out, "mpc_amd.hip"], cwd=capi.CSRC)
    return _isa_loops().analyse(out, KERNEL)


@pytest.fixture(scope="module")
def parent():
    with open(os.path.join(ROOT, "profiles", "wv_sweep_gaps_isa_before.json")) as fh:
        before = json.load(fh)
    assert tuple(s["instrs"] for s in before["tile_sweeps"]) == PARENT_INSTRS
    return before


def test_fewer_products_back_to_back_and_no_more_instructions_per_trip(listing, parent):
    sweeps, before = listing["tile_sweeps"], parent["tile_sweeps"]
    assert len(sweeps) == 4 and len(before) == 4, ([s["head"] for s in sweeps], [s["head"] for s in before])
    for s, b in zip(sweeps, before):
        print({k: (b[k], s[k]) for k in ("instrs", "mfma", "mfma_adjacent", "nop", "lds", "valu", "wait")})
    for s, b in zip(sweeps, before):
        assert s["mfma"] == b["mfma"], (s, b)      # the same products
        assert s["mfma_adjacent"] < b["mfma_adjacent"], (s, b)
        assert s["nop"] <= b["nop"], (s, b)
        assert s["instrs"] <= b["instrs"], (s, b)


def test_no_private_segment(listing):
    print(listing["resources"])
    assert listing["resources"]["private_seg_size"] == 0, listing["resources"]
