"""The host layer the three libraries share (csrc/mpc_host.hpp) and the one list of sources their builds depend on - both without a GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "mpc-code_amd", "csrc")


def test_soa_staging_log_layout_and_range_checks_under_sanitizers(tmp_path):
    """tests/host_layer_check.cpp - a program of its own that includes mpc_host.hpp and makes no HIP call - with its host side under ASan and UBSan, run as a
    child process: to_soa -> from_soa round trips with zero padding lanes (B in {1, 63, 64, 65, 130}, d in {0, 1, 3}), the log table's layout against the closed
    forms of the three alloc functions, the [k0, k0 + n) range check; and the un-padding of a gathered [2][2][3][128] block for B = 65 against numpy."""
    exe = str(tmp_path / "host_layer_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "host_layer_check.cpp")], check=True)
    blk = np.random.default_rng(11).standard_normal((2, 2, 3, 128))
    blk.tofile(tmp_path / "block.bin")
    r = subprocess.run([exe, str(tmp_path / "block.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0 and "host layer ok" in r.stdout, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    got = np.fromfile(tmp_path / "out.bin").reshape(2, 2, 65, 3)
    assert np.array_equal(got, blk[..., :65].transpose(0, 1, 3, 2))


@pytest.fixture
def source_copy(pkg, tmp_path, monkeypatch):
    """the package's build recipes looking at a copy of the sources (csrc/*.hip, csrc/*.hpp, include/*.h): the test edits the copy, not the tree"""
    from mpc_code_amd import capi
    (tmp_path / "pkg" / "csrc").mkdir(parents=True)
    (tmp_path / "include").mkdir()
    for f in capi.source_files():
        shutil.copy2(f, tmp_path / ("include" if f.endswith(".h") else os.path.join("pkg", "csrc")))
    monkeypatch.setattr(capi, "PKG_DIR", str(tmp_path / "pkg"))
    monkeypatch.setattr(capi, "CSRC", str(tmp_path / "pkg" / "csrc"))
    return tmp_path


def test_one_source_list_feeds_the_freshness_test_and_both_hashes(pkg, source_copy):
    """An edit to any header a library includes rebuilds it: mpc_soft.hpp (which the old hand-written lists left out) makes a cached linear library stale
    by its time stamp, and moves the hashed names of the per-model libraries by its content."""
    from mpc_code_amd import capi, econcodegen, nlcodegen
    files = capi.source_files()
    assert all(os.path.dirname(f).startswith(str(source_copy)) for f in files)
    names = {os.path.basename(f) for f in files}
    assert {"mpc_soft.hpp", "mpc_comm.hpp", "mpc_host.hpp", "mpc_amd.h", "mpc_nmpc.h", "mpc_enmpc.h", "mpc_amd.hip", "mpc_nmpc.hip", "mpc_enmpc.hip"} <= names
    real = {os.path.basename(f) for d, ext in ((CSRC, (".hip", ".hpp")), (os.path.join(ROOT, "include"), (".h",))) for f in os.listdir(d) if f.endswith(ext)}
    assert names == real      # every csrc/*.hip, csrc/*.hpp and include/*.h, and nothing from csrc/jit/
    lib = source_copy / "libmpc_amd.so"
    lib.write_bytes(b"")
    newest = max(os.path.getmtime(f) for f in files)
    os.utime(lib, (newest + 10, newest + 10))
    assert capi.library_is_fresh(str(lib))
    soft = source_copy / "pkg" / "csrc" / "mpc_soft.hpp"
    nl0, ec0 = nlcodegen.nmpc_library_path("model"), econcodegen.enmpc_library_path("model")
    assert nl0 == nlcodegen.nmpc_library_path("model") and ec0 == econcodegen.enmpc_library_path("model")
    os.utime(soft, (newest + 20, newest + 20))      # touched
    assert not capi.library_is_fresh(str(lib))
    assert not capi.library_is_fresh(str(source_copy / "absent.so"))
    with open(soft, "a") as fh:                     # ... and edited
        fh.write("// edited\n")
    assert nlcodegen.nmpc_library_path("model") != nl0 and econcodegen.enmpc_library_path("model") != ec0
