"""Vector-memory waits and dead work inside a step of the wave-autonomous loop kernel, read from a cross-compiled listing (no GPU).

With the last block's cost weight selected from scalar-loaded values, the tile constants of one-tile stages in LDS and the one-wave
synchronisation that orders LDS only, the interior-point iteration of the headline kernel holds no vector-memory load and no wait with
a vmcnt field; it and the kernel as a whole hold fewer instructions than at the parent commit
(profiles/wv_step_stalls_isa_before.json, made by tools/isa_loops.py from the parent's listing), on no more registers and without a
private segment.  The maxima with two equal sources (the copy that quiets an operand of a maximum or minimum) are counted against the
change's own committed record, profiles/wv_step_stalls_isa.json."""
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
BEFORE = os.path.join(ROOT, "profiles", "wv_step_stalls_isa_before.json")
RECORD = os.path.join(ROOT, "profiles", "wv_step_stalls_isa.json")


def _isa_loops():
    spec = importlib.util.spec_from_file_location("isa_loops", os.path.join(ROOT, "tools", "isa_loops.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def iteration_loop(listing):
    """The interior-point iteration, found as in tests/test_wv_lane_phase_isa.py: the smallest reported loop that contains all four
    tile sweeps (labels are numbered in program order)."""
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
    out = str(tmp_path_factory.mktemp("wv_step_stalls_isa") / "mpc_amd_cstr.s")
    flags = [f for f in capi.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    flags.append("-DMPC_DIM_LIST(X)=X(" + ",".join(str(v) for v in CSTR_DIMS) + ")")
    subprocess.check_call([HIPCC] + flags + ["--offload-device-only", "-S", "-o", out, "mpc_amd.hip"], cwd=capi.CSRC)
    return _isa_loops().analyse(out, KERNEL)


@pytest.fixture(scope="module")
def before():
    with open(BEFORE) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def record():
    with open(RECORD) as fh:
        return json.load(fh)


def test_the_counters_tell_the_instructions_apart():
    m = _isa_loops()
    assert m.extras("global_load_dwordx4", "global_load_dwordx4 v[0:3], v[4:5], off") == ["vmem_load"]
    assert m.extras("flat_load_dword", "flat_load_dword v0, v[4:5]") == ["vmem_load"]
    assert m.extras("global_store_dwordx2", "global_store_dwordx2 v[4:5], v[0:1], off") == []
    assert m.extras("s_waitcnt", "s_waitcnt vmcnt(0) lgkmcnt(0)") == ["vmcnt_wait"]
    assert m.extras("s_waitcnt", "s_waitcnt lgkmcnt(0)") == []
    assert m.extras("v_max_f64", "v_max_f64 v[0:1], v[2:3], v[2:3]") == ["canon_max"]
    assert m.extras("v_max_f64", "v_max_f64 v[0:1], v[2:3], v[4:5]") == []
    assert m.extras("v_max_f64", "v_max_f64 v[0:1], |v[2:3]|, |v[2:3]|") == ["canon_max"]


def test_no_vector_memory_load_and_no_vmcnt_wait_inside_the_iteration(listing, before):
    now, then = iteration_loop(listing), iteration_loop(before)
    print("iteration loop: vmem_load", then["vmem_load"], "->", now["vmem_load"], "| vmcnt_wait", then["vmcnt_wait"], "->", now["vmcnt_wait"])
    assert then["vmem_load"] > 0 and then["vmcnt_wait"] > 0, then      # the parent's record is of the same counters
    assert now["vmem_load"] == 0, now
    assert now["vmcnt_wait"] == 0, now


def test_iteration_loop_and_kernel_are_shorter_than_the_parents(listing, before):
    now, then = iteration_loop(listing), iteration_loop(before)
    print("iteration loop", then["instrs"], "->", now["instrs"], "| kernel", before["total"]["instrs"], "->", listing["total"]["instrs"])
    assert now["instrs"] < then["instrs"], (now, then)
    assert listing["total"]["instrs"] < before["total"]["instrs"], (listing["total"], before["total"])


def test_no_more_registers_and_no_private_segment(listing, before):
    res, was = listing["resources"], before["resources"]
    print(was, "->", res)
    assert res["private_seg_size"] == 0, res
    assert listing["total"]["scratch"] == 0, listing["total"]
    assert res["num_vgpr"] <= was["num_vgpr"] and res["num_agpr"] <= was["num_agpr"], (res, was)


def test_canonicalising_maxima_are_those_of_the_record(listing, before, record):
    print("canon_max: parent", before["total"]["canon_max"], "| record", record["total"]["canon_max"], "| listing", listing["total"]["canon_max"],
          "| iteration loop", iteration_loop(before)["canon_max"], "->", iteration_loop(listing)["canon_max"])
    assert record["total"]["canon_max"] < before["total"]["canon_max"], (record["total"], before["total"])
    assert listing["total"]["canon_max"] == record["total"]["canon_max"], (listing["total"], record["total"])
    assert iteration_loop(listing)["canon_max"] == iteration_loop(record)["canon_max"]
