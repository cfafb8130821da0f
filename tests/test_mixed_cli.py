"""spmv-csr / spmv-csrk --vector-dtype: the mixed handle (fp32 values read from
the file, fp64 x and y) through the command-line drivers, and the library's
refusal of the other unequal pair."""
import subprocess

import numpy as np
import pytest

import hspmv
from conftest import REPO
from hspmv import gen

BUILD = REPO / "heterogeneous-spmv_amd" / "build"


def run(*args):
    return subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)


def test_usage_names_the_option():
    assert "--vector-dtype" in run(BUILD / "spmv-csr").stdout


@pytest.fixture(scope="module")
def stencil_file(tmp_path_factory):
    assert hspmv.device_count() >= 1, "no HIP device visible: the gpu tests must run on the MI355X box"
    f = tmp_path_factory.mktemp("mixed_cli") / "stencil12.csr"
    gen.write_csr_text(str(f), gen.stencil27(12))
    return f


@pytest.mark.gpu
def test_spmv_csr_mixed_dumps_the_python_handles_y(stencil_file, tmp_path):
    out = tmp_path / "y.bin"
    p = run(BUILD / "spmv-csr", stencil_file, 5, "--dtype", "f32", "--vector-dtype", "f64", "--dump-y", out)
    assert p.returncode == 0, p.stdout + p.stderr
    for key in ("TimeMin:", "TimeMax:", "TimeAvg:"):
        assert key in p.stdout
    assert "Number Wrong: 0" in p.stdout and "Check: PASS" in p.stdout  # the fp64 host sum of the widened values
    A = hspmv.read_csr(stencil_file, np.float32)  # the file's values, rounded to fp32 as the driver reads them
    assert out.stat().st_size == 8 * A.m
    y = np.fromfile(out, np.float64)
    with hspmv.SpMV(A, vector_dtype=np.float64) as op:
        want = op(np.ones(A.n))
    assert y.tobytes() == want.tobytes()
    # x = rand and the CSR-3 driver: the same contract
    p = run(BUILD / "spmv-csrk", stencil_file, 5, 20, 10, "--file-order", "--dtype", "f32", "--vector-dtype", "f64",
            "--x", "rand:42", "--dump-y", out)
    assert p.returncode == 0 and "Check: PASS" in p.stdout, p.stdout + p.stderr
    y = np.fromfile(out, np.float64)
    with hspmv.SpMV(A, hspmv.build_csr3_maps(A, 20, 10), vector_dtype=np.float64) as op:
        want = op(gen.rand_x(A.n, 42))
    assert y.tobytes() == want.tobytes()


@pytest.mark.gpu
def test_spmv_csr_refuses_fp64_values_with_fp32_vectors(stencil_file):
    p = run(BUILD / "spmv-csr", stencil_file, 5, "--dtype", "f64", "--vector-dtype", "f32")
    assert p.returncode != 0
    assert "fp64 values with fp32 vectors" in p.stderr  # the library's message
    p = run(BUILD / "spmv-csr", stencil_file, 5, "--dtype", "f32", "--vector-dtype", "f64", "--gpus", "2")
    assert p.returncode != 0 and "one device" in p.stderr
    p = run(BUILD / "spmv-csr", stencil_file, 5, "--dtype", "f32", "--vector-dtype", "f16")
    assert p.returncode != 0
