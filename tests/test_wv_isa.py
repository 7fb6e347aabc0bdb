"""The instruction stream of the wave-autonomous loop kernel, read from a cross-compiled listing (no GPU): the tile sweeps of
mpc_wave.hpp run their matrix-core products in VGPR form - no accumulator moves, no scratch - and the kernel still fits its launch."""
import importlib.util
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSTR_DIMS = (3, 2, 3, 3, 3, 0, 0)      # the benchmark's dimension set (examples/cstr_lmpc.py)
# loop_kernel_wv<NX, NU, NY, ND, NXP, HASM, GR, NC, MASKED, NI = 4, ...>: four instances per wave, every bound finite
KERNEL = "loop_kernel_wvILi3ELi2ELi3ELi3ELi3ELb0ELi0ELi5ELb0ELi4E"
PARENT_PRIVATE_SEGMENT = 12             # bytes, before the products moved to VGPR form


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
    out = str(tmp_path_factory.mktemp("wv_isa") / "mpc_amd_cstr.s")
    flags = [f for f in capi.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    flags.append("-DMPC_DIM_LIST(X)=X(" + ",".join(str(v) for v in CSTR_DIMS) + ")")
    subprocess.check_call([HIPCC] + flags + ["--offload-device-only", "-S", "-o", out, "mpc_amd.hip"], cwd=capi.CSRC)
    return _isa_loops().analyse(out, KERNEL)


def test_tile_sweeps_hold_no_accumulator_moves_and_no_scratch(listing):
    sweeps = listing["tile_sweeps"]
    for s in sweeps:
        print(s)
    # tile_factor, tile_forward (predictor), tile_rhs, tile_forward (corrector): the self-looping blocks that hold v_mfma_f64
    assert len(sweeps) == 4, [s["head"] for s in sweeps]
    for s in sweeps:
        assert s["mfma"] > 0 and s["mfma"] % 4 == 0, s      # groups of four blocks
        assert s["accvgpr"] == 0, s
        assert s["scratch"] == 0, s


def test_kernel_still_fits_its_launch(listing):
    res = listing["resources"]
    print(res, listing["total"])
    assert res["private_seg_size"] <= PARENT_PRIVATE_SEGMENT, res
    # __launch_bounds__(64, 1): one wave per SIMD owns the whole register file, 256 architectural + 256 accumulation registers
    assert res["num_vgpr"] <= 256 and res["num_agpr"] <= 256, res
