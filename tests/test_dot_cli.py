"""spmv-csr --dot: hspmv_spmv_axpby_dot through the command-line driver, with
and without --axpby, on a matrix of short rows (the row slices' shape) and on
a Laplacian; the refusals that are decided while the arguments are parsed."""
import re
import subprocess

import numpy as np
import pytest

import hspmv
from conftest import REPO
from dot_cases import ragged_lengths
from hspmv import gen

BUILD = REPO / "heterogeneous-spmv_amd" / "build"


def run(*args):
    return subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)


def test_usage_names_the_option():
    assert "--dot" in run(BUILD / "spmv-csr").stdout


def test_refusals_come_before_anything_is_read():
    p = run(BUILD / "spmv-csr", "/does/not/exist.csr", 3, "--rhs", 4, "--dot")
    assert p.returncode == 1 and "--rhs takes no --dot" in p.stderr and "Before Read" not in p.stdout
    p = run(BUILD / "spmv-csr", "/does/not/exist.csr", 3, "--gpus", 2, "--dot")
    assert p.returncode == 1 and "--dot runs on one GPU" in p.stderr and "Before Read" not in p.stdout


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    assert hspmv.device_count() >= 1, "no HIP device visible: the gpu tests must run on the MI355X box"
    d = tmp_path_factory.mktemp("dot_cli")
    out = {}
    for name, A in (("short_rows", ragged_lengths(700, np.float64, seed=51)), ("lap", gen.laplace2d(40, 30))):
        f = d / f"{name}.csr"
        gen.write_csr_text(str(f), A)
        out[name] = f
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["short_rows", "lap"])
@pytest.mark.parametrize("extra", [[], ["--axpby", "-1,0.5"]], ids=["plain", "axpby"])
def test_gpu_dot_check_passes_on_the_path_the_handle_reports(files, name, extra):
    f = files[name]
    with hspmv.SpMV(hspmv.read_csr(f, np.float64), device=0) as op:  # the driver's handle: every choice the library's
        path = op.axpby_path
    p = run(BUILD / "spmv-csr", f, 4, "--x", "rand:42", *extra, "--dot")
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"^DotCheck: (\w+) wy=(\S+) yy=(\S+) path=(\w+)$", p.stdout, re.M)
    assert m, p.stdout
    assert m.group(1) == "PASS" and m.group(4) == path
    assert np.isfinite(float(m.group(2))) and float(m.group(3)) > 0.0
    for key in ("DotTimeMin:", "DotTimeMax:", "DotTimeAvg:", "DotKernelMin:"):
        assert re.search(rf"^{key} \S+$", p.stdout, re.M), key
    assert ("AxpbyCheck: PASS" in p.stdout) == bool(extra)
    assert "Check: PASS" in p.stdout
