"""The lane-per-block phases of the wave-autonomous loop kernel, read from a cross-compiled listing (no GPU): with lane votes for the
maxima that are only compared and DPP moves without an `old` operand, the interior-point iteration and the kernel as a whole hold fewer
instructions than at the parent commit (profiles/wv_lane_phase_isa_before.json, made by tools/isa_loops.py from the parent's listing),
and nothing was traded for registers or scratch."""
import importlib.util
import json
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSTR_DIMS = (3, 2, 3, 3, 3, 0, 0)      # the benchmark's dimension set (examples/cstr_lmpc.py)
KERNEL = "loop_kernel_wvILi3ELi2ELi3ELi3ELi3ELb0ELi0ELi5ELb0ELi4E"      # as in tests/test_wv_isa.py
BEFORE = os.path.join(ROOT, "profiles", "wv_lane_phase_isa_before.json")


def _isa_loops():
    spec = importlib.util.spec_from_file_location("isa_loops", os.path.join(ROOT, "tools", "isa_loops.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def iteration_loop(listing):
    """The interior-point iteration: the smallest reported loop that contains all four tile sweeps.  Labels are numbered in program
    order, so a loop contains a sweep when the sweep's label lies between its head and its tail."""
    def num(label):
        return tuple(int(v) for v in label[len(".LBB"):].split("_"))
    sweeps = listing["tile_sweeps"]
    assert len(sweeps) == 4, [s["head"] for s in sweeps]
    holds = [l for l in listing["loops"] if not l["self_loop"] and all(num(l["head"]) <= num(s["head"]) <= num(l["tail"]) for s in sweeps)]
    assert holds, "no loop holds the four tile sweeps"
    return min(holds, key=lambda l: l["instrs"])


@pytest.fixture(scope="module")
def listing(pkg, tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc: the listing cannot be made")
    from mpc_code_amd import capi
    out = str(tmp_path_factory.mktemp("wv_lane_isa") / "mpc_amd_cstr.s")
    flags = [f for f in capi.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    flags.append("-DMPC_DIM_LIST(X)=X(" + ",".join(str(v) for v in CSTR_DIMS) + ")")
    subprocess.check_call([HIPCC] + flags + ["--offload-device-only", "-S", "-o", out, "mpc_amd.hip"], cwd=capi.CSRC)
    return _isa_loops().analyse(out, KERNEL)


@pytest.fixture(scope="module")
def before():
    with open(BEFORE) as fh:
        return json.load(fh)


def test_iteration_loop_and_kernel_are_shorter_than_the_parents(listing, before):
    now, then = iteration_loop(listing), iteration_loop(before)
    print("iteration loop", then["instrs"], "->", now["instrs"], "| kernel", before["total"]["instrs"], "->", listing["total"]["instrs"])
    assert now["instrs"] < then["instrs"], (now, then)
    assert listing["total"]["instrs"] < before["total"]["instrs"], (listing["total"], before["total"])


def test_nothing_was_traded_for_registers_or_scratch(listing):
    res = listing["resources"]
    print(res)
    assert res["private_seg_size"] == 0, res
    assert listing["total"]["scratch"] == 0, listing["total"]
    assert res["num_vgpr"] <= 256 and res["num_agpr"] <= 256, res
