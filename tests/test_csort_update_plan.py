"""The column-sorted value refresh on the CPU (plan_csort's source-index table,
csrc/hspmv_csort_build.cpp; the kernels of csrc/refresh.hip restated on the
host).

tools/csort_update_check.cpp plans each of some seventy small matrices -- the
shape families of csort_plan_check: both dtypes, wide and narrow layouts, one,
two and four column parts, segmented chunks, sliced and whole long rows,
fixed-point scales, chunks closed early on the 65535-column span, empty rows --
with values v0 and the source table, restates the two refresh kernels over
independent values v1 (rows that become zero, rows that were zero, rows
rescaled by 2^+-40, a row spanning more than 2^100) and requires the result to
be plan_csort(v1) byte for byte; its header lists every assertion.
"""
import re
import subprocess

from conftest import REPO

CHECK = REPO / "heterogeneous-spmv_amd" / "build" / "csort_update_check"


def test_refresh_restated_on_the_host_equals_a_new_plan():
    p = subprocess.run([str(CHECK)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    m = re.search(r"^csort_update_check: (\d+) cases ok$", p.stdout, re.M)
    assert m and int(m.group(1)) >= 60, p.stdout[-500:]
