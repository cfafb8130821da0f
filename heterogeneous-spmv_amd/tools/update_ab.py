#!/usr/bin/env python3
"""What new values cost on a planned handle (hspmv_update_values) against the
only alternative before it: destroy + create of the same handle.

    python heterogeneous-spmv_amd/tools/update_ab.py [--parent-lib OLD/libhspmv.so.1]
           [--cases c3,c3mixed,c5det] [--rounds 5] [--out profiles/update_values/update_ab.jsonl]

In one process, per case (the bench's C3 handle in fp64 and mixed: row slices;
C5 with deterministic = 1: x slabs; c5csort / c5csort_det2: C5 fp32 with the
default plan, the column-sorted kernel, and the same with deterministic = 2,
on a handle from hspmv_create_updatable), minima over ``--rounds``:
  (a) device   update_values_device from a resident device array, HIP events
               on the handle's stream;
  (b) host     update_values from (pageable) host memory, wall time;
  (c) recreate hspmv_destroy + the same create call from host arrays, wall
               time -- through ``--parent-lib`` (a build of the commit before
               the update entry points, loaded privately as tools/ab.py does)
               when given, else through this build, whose create path is the
               same code.
For (a) the line carries the bytes the update reads and writes and what
fraction of 8 TB/s that is, and for each of (a)-(c) the round-to-round spread
(max - min).  After the timed rounds y of the updated handle is compared bit
for bit with a fresh handle's over the same values (a column-sorted handle
without fixed-point slots adds in atomic order: there the line says whether y
is within 1e-4 |y| + 1e-5 sum|a x| of it).  The column-sorted cases also run
hspmv_run of the updatable handle and of a plain one alternately, ``--rounds``
times each: the same kernel over the same tables, so the difference of the
minima should stay inside the plain handle's own spread.
"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE))

import torch  # noqa: E402  (load order: torch's HIP runtime first)

import hspmv  # noqa: E402
from hspmv import _lib, gen  # noqa: E402
from ab import load  # noqa: E402
import sweep  # noqa: E402

HBM_PEAK = 8.0e12


def case(name):
    """(A, maps, SpMV keyword arguments, what info must show)"""
    if name == "c3":
        A, maps, _ = sweep.build("c3")
        return A, maps, {}, ("row_slices", 1)
    if name == "c3mixed":
        A, maps, _ = sweep.build("c3")
        return A.astype(np.float32), maps, {"vector_dtype": np.float64}, ("row_slices", 1)
    if name == "c5det":
        A, maps, _ = sweep.build("c5")
        return A, maps, {"options": {"deterministic": 1}}, ("x_slabs", None)
    if name == "c5csort":
        A, maps, _ = sweep.build("c5")
        return A, maps, {"updatable": True}, ("kernel_name", "csort")
    if name == "c5csort_det2":
        A, maps, _ = sweep.build("c5")
        return A, maps, {"updatable": True, "options": {"deterministic": 2}}, ("kernel_name", "csort")
    raise ValueError(name)


def update_bytes(A, maps, kw, info):
    """Bytes the device update reads + writes (the model of DESIGN.md 5d)."""
    sv = A.val.dtype.itemsize
    if info["row_slices"]:
        S = hspmv.slices_plan(A, maps, options=kw.get("options"), fill=False,
                              vector_dtype=kw.get("vector_dtype"))
        rd = A.nnz * sv + 4 * (A.m + 1) + A.m + 8 * (S["n_desc"] + 1)
        return rd, S["padded_entries"] * sv
    rd, wr = A.nnz * sv, A.nnz * sv  # the copy into the CSR-order values
    if info["kernel_name"] == "csort":
        # per stored entry (padding included): its source index, the {idx, val}
        # record read and written (fp64: the value written; the index word read
        # under fixed-point slots only), and the gathered CSR-order value
        P = info["csort_chunks"] * 64 * info["chunk_u"]
        fixed = info["csort_fixed_point"]
        rd += 4 * P + (8 * P if sv == 4 else (4 * P if fixed else 0)) + A.nnz * sv
        wr += 8 * P
        if fixed:  # the row scales: the values and the row pointers once more, rexp written, then gathered
            rd += A.nnz * sv + 4 * (A.m + 1) + 2 * A.nnz
            wr += 2 * A.m
    if info["x_slabs"]:
        rd += A.nnz * sv + 4 * (A.m + 1) * (1 + info["x_slabs"])
        wr += A.nnz * sv
    return rd, wr


def recreate_wall(L, A, maps, kw, rounds):
    """(min, max - min) wall seconds of destroy + create (+ synchronize) through library L."""
    cs, ms = A.c_struct(), maps.c_struct()
    opt = _lib.make_options(0, kw.get("options"), device=0)
    mixed = kw.get("vector_dtype") is not None

    def create():
        h = C.c_void_p()
        if mixed:
            rc = L.hspmv_create_mixed(C.byref(h), C.byref(cs), C.byref(ms), C.byref(opt), _lib.F64)
        else:
            rc = L.hspmv_create_ex(C.byref(h), C.byref(cs), C.byref(ms), C.byref(opt))
        assert rc == 0, L.hspmv_last_error()
        return h

    h, ts = create(), []
    for _ in range(rounds):
        tic = time.perf_counter()
        L.hspmv_destroy(h)
        h = create()
        assert L.hspmv_synchronize(h) == 0
        ts.append(time.perf_counter() - tic)
    L.hspmv_destroy(h)
    return min(ts), max(ts) - min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--cases", default="c3,c3mixed,c5det")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--tag", default="", help="names the library under test in the lines (HSPMV_LIB picks it)")
    ap.add_argument("--no-recreate", action="store_true", help="skip (c)")
    a = ap.parse_args()
    parent = load(a.parent_lib) if a.parent_lib else None
    stream = torch.cuda.Stream()
    out = []
    for name in a.cases.split(","):
        A, maps, kw, (key, want) = case(name)
        xdt = kw.get("vector_dtype", A.val.dtype)
        x = gen.rand_x(A.n, 42).astype(xdt)
        rng = np.random.default_rng(7)
        v_new = rng.uniform(-1.0, 1.0, A.nnz).astype(A.val.dtype)
        t_new = torch.from_numpy(v_new).cuda()
        torch.cuda.synchronize()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with hspmv.SpMV(A, maps, device=0, stream=stream.cuda_stream, **kw) as op:
            info = op.info
            if not (info[key] == want if want is not None else info[key] >= 2):
                print(f"# {name}: expected {key} = {want or '>= 2'}, the handle reports {info[key]}", flush=True)
            op.set_x(x)
            op.spmv()
            op.synchronize()
            dev, host = [], []
            for _ in range(a.rounds):
                ev0.record(stream)
                op.update_values_device(t_new.data_ptr())
                ev1.record(stream)
                ev1.synchronize()
                dev.append(ev0.elapsed_time(ev1) * 1e-3)
                tic = time.perf_counter()
                op.update_values(v_new)
                host.append(time.perf_counter() - tic)
            op.spmv()
            y = op.get_y()
            assert op.info == info
            run_ab = None
            if kw.get("updatable"):  # the SpMV itself: this handle against a plain one, alternately
                plain_kw = {k: v for k, v in kw.items() if k != "updatable"}
                with hspmv.SpMV(hspmv.CsrMatrix(A.m, A.n, A.row_ptr, A.col_idx, v_new), maps, device=0,
                                **plain_kw) as plain:
                    plain.set_x(x)
                    tu, tp = [], []
                    for _ in range(a.rounds):
                        tp.append(plain.run(3, 20)["t_min"])
                        tu.append(op.run(3, 20)["t_min"])
                    run_ab = {"updatable_us": round(min(tu) * 1e6, 2), "plain_us": round(min(tp) * 1e6, 2),
                              "updatable_spread_us": round((max(tu) - min(tu)) * 1e6, 2),
                              "plain_spread_us": round((max(tp) - min(tp)) * 1e6, 2),
                              "device_bytes_updatable": info["device_bytes"],
                              "device_bytes_plain": plain.info["device_bytes"]}
        fresh_kw = {k: v for k, v in kw.items() if k != "updatable"}
        with hspmv.SpMV(hspmv.CsrMatrix(A.m, A.n, A.row_ptr, A.col_idx, v_new), maps, device=0, **fresh_kw) as fresh:
            y_fresh = fresh(x)
            y_equal = bool(np.array_equal(y_fresh.view(np.uint8), y.view(np.uint8)))
        y_close = None
        if not y_equal:
            rows = np.repeat(np.arange(A.m), np.diff(A.row_ptr))
            absrow = np.bincount(rows, np.abs(v_new.astype(np.float64)) * np.abs(x[A.col_idx]), minlength=A.m)
            y_close = bool(np.all(np.abs(y.astype(np.float64) - y_fresh) <= 1e-4 * np.abs(y_fresh) + 1e-5 * absrow))
        t_re, t_re_spread = (float("nan"), float("nan")) if a.no_recreate else \
            recreate_wall(parent if parent is not None else _lib.lib(), A, maps, fresh_kw, a.rounds)
        rd, wr = update_bytes(A, maps, kw, info)
        rec = {"case": name, "lib": a.tag or Path(_lib.LIB_PATH).parent.name + "/" + Path(_lib.LIB_PATH).name, "m": A.m, "nnz": A.nnz, "value_dtype": str(A.val.dtype), "vector_dtype": str(np.dtype(xdt)),
               "kernel": info["kernel_name"], "row_slices": info["row_slices"], "x_slabs": info["x_slabs"],
               "device_update_us": round(min(dev) * 1e6, 2), "host_update_ms": round(min(host) * 1e3, 3),
               "recreate_ms": None if a.no_recreate else round(t_re * 1e3, 3), "recreate_lib": "parent" if parent is not None else "this",
               "bytes_read": int(rd), "bytes_written": int(wr),
               "device_update_frac_of_8TBps": round((rd + wr) / min(dev) / HBM_PEAK, 4),
               "device_update_spread_us": round((max(dev) - min(dev)) * 1e6, 2),
               "host_update_spread_ms": round((max(host) - min(host)) * 1e3, 3),
               "recreate_spread_ms": None if a.no_recreate else round(t_re_spread * 1e3, 3),
               "rounds": a.rounds, "y_equal_fresh": y_equal, "y_close_fresh": y_close, "run_ab": run_ab}
        out.append(rec)
        print(json.dumps(rec), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("".join(json.dumps(r) + "\n" for r in out))


if __name__ == "__main__":
    main()
