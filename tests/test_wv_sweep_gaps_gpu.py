"""The pipelined tile sweeps of the wave solver (csrc/mpc_wave.hpp, one-tile stages with constant matrices) against the generic path of
the same products, bit for bit: the library built with -DMPC_WV_GENERIC_TILES, as in tests/test_wv_directions.py, at the horizons where
a sweep that is skewed by one block and reads the next group's operands from inside its statements can go wrong:

    N = 2                            no full group: the opening statement and the blocks left over only
    N = 4, 5, 7, 8, 9, 11, 12, 13    one to three full groups with each remainder (first, steady and last trip differ)
    N = 64                           the longest horizon: the look-ahead reads of the last group at the end of the LDS allocation

on the benchmark's dimension set, on NU = 1 (the second row of Lambda is read from the row of zeros) and on NS = 4 (kff has a store of
its own), and on the other three sets whose sweeps take this path (tests/wv_direction_ref.py:VGPR_SETS - each set is a kernel with a
register allocation of its own, and the reads issued from inside the statements rely on no register being moved before their wait),
with batches 7, 2 and 1 (waves with dead tiles), full solves and solves cut after 1..4 iterations.  Every bound is finite (the
kernels without bound masks, the benchmark's; the set with a general output row has the masked kernels only): the masks do not reach
the sweeps.  Every bit of status, iters, u0, x1, w and res has to be equal.  Both libraries of each set are built by build(); nothing
is compiled here.
"""
import copy
import os

import numpy as np
import pytest

import wv_direction_ref as wd

pytestmark = pytest.mark.gpu

SETS = [(3, 2, 3, 3, 3, 0, 0), (1, 1, 1, 1, 1, 0, 0), (4, 2, 2, 2, 4, 0, 0)]
SETS += [d for d in wd.VGPR_SETS if d not in SETS]
HORIZONS = [2, 4, 5, 7, 8, 9, 11, 12, 13, 64]
BATCHES = (7, 2, 1)
CASES = [(d, N) for d in SETS for N in HORIZONS]
assert all(d in wd.VGPR_SETS for d in SETS)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


@pytest.mark.parametrize("dims,N", CASES, ids=[f"{wd.set_id(d)}-N{N}" for d, N in CASES])
def test_pipelined_sweeps_equal_the_generic_path_bit_for_bit(dims, N, solver_factory):
    from mpc_code_amd import capi
    finite = not dims[6]
    p = wd.direction_problem(dims, N, finite)
    generic = capi.build_library(dims=dims, extra_flags=wd.GENERIC_TILES)      # built by build(); here only its path
    assert os.path.basename(generic) != os.path.basename(capi.jit_library_path(dims))
    made = []
    try:
        for mi in (None, 1, 2, 3, 4):
            q = copy.copy(p)
            if mi is not None:
                q.max_iter = mi
            a = solver_factory(q); made.append(a); a.set_option("ocp_kernel", 3)
            b = capi.Solver(q, device=0, lib_path=generic); made.append(b); b.set_option("ocp_kernel", 3)
            assert "wv_generic_tiles" in b.build_info().split(";") and "wv_generic_tiles" not in a.build_info().split(";"), (a.build_info(), b.build_info())
            for B in BATCHES:
                inp = wd.direction_inputs(p, B, wd.case_seed(dims, N, finite) + B)
                ga, gb = a.ocp_solve(*inp, want_w=True), b.ocp_solve(*inp, want_w=True)
                if mi is not None:
                    assert (ga["status"] == 1).all() and (ga["iters"] == mi).all(), (mi, B, ga["status"], ga["iters"])
                for k in ("status", "iters", "u0", "x1", "w", "res"):
                    same = _bits(ga[k]) == _bits(gb[k])
                    assert same.all(), (mi, B, k, np.argwhere(~same)[:8], ga[k][~same][:8], gb[k][~same][:8])
    finally:
        for s in made:
            s.close()
