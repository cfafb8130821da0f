"""The row kernels' host tables on the CPU (csrc/hspmv_tables.cpp).

tools/row_tables_check.cpp plans some ninety small cases -- the 16-bit
columns with block bases (the base-block and plane-word edges, 0 / 1 / 2 / 8
/ 9 planes, NO_COL16, resident and not, both vector dtypes) and with group
bases (m of 1 / 64 / 65, the 65535 / 65536 span, a split row, an empty
group, task starts, the three modes), the x slabs (forced B with n no
multiple of it, the clips, descending rows, a split row, empty rows, both
value dtypes, the exits), the split rows (4096 / 4097 / 8192 / 8193
nonzeros, NO_SPLIT), the two rules of build_row_tables and the bytes-saved
formulas -- decodes every table back into the matrix the way the kernels
read it (its header lists what it requires) and prints one line per case:
the scalars, the bytes saved as a hex float and an FNV-1a 64 digest of each
array.  The lines below were recorded from the functions these planners were
split out of (profiles/row_tables_plan/parent_digests.txt says how): a
change to them is a change to the bytes the kernels are given, which the GPU
parity tests then have to justify.
"""
import subprocess

from conftest import REPO

CHECK = REPO / "heterogeneous-spmv_amd" / "build" / "row_tables_check"

EXPECTED = """\
blocks_nnz1 col16 taken=1 mode=1 planes=0 words=2 span_bits=1 shape=0 saved=-0x1p+1 off=08328807b4eb6fed base=0e0a0a27a32b9948 planes=cbf29ce484222325
blocks_nnz65 col16 taken=1 mode=1 planes=0 words=3 span_bits=8 shape=0 saved=0x1.f8p+6 off=9b3ed0e709969d91 base=0e0a0a27a32b9948 planes=cbf29ce484222325
blocks_plane_nnz65 col16 taken=1 mode=1 planes=1 words=3 span_bits=17 shape=0 saved=0x1.d78p+6 off=b697adabe0b64712 base=0e0a0a27a32b9948 planes=f6a3474cf25deec5
blocks_nnz129 col16 taken=1 mode=1 planes=0 words=4 span_bits=9 shape=0 saved=0x1.fcp+7 off=910ccd99d4a609ea base=0e0a0a27a32b9948 planes=cbf29ce484222325
blocks_plane_nnz129 col16 taken=1 mode=1 planes=1 words=4 span_bits=17 shape=0 saved=0x1.dbcp+7 off=2180eab0bd19e511 base=0e0a0a27a32b9948 planes=76fca43424299bb5
blocks_nnz255 col16 taken=1 mode=1 planes=0 words=5 span_bits=10 shape=0 saved=0x1.fap+8 off=eabe08f5ef5f2531 base=0e0a0a27a32b9948 planes=cbf29ce484222325
blocks_plane_nnz255 col16 taken=1 mode=1 planes=1 words=5 span_bits=17 shape=0 saved=0x1.da2p+8 off=56251549d9f62d45 base=0e0a0a27a32b9948 planes=7613e7eadc45af4d
blocks_nnz256 col16 taken=1 mode=1 planes=0 words=5 span_bits=10 shape=0 saved=0x1.fcp+8 off=86727d6300168597 base=0e0a0a27a32b9948 planes=cbf29ce484222325
blocks_plane_nnz256 col16 taken=1 mode=1 planes=1 words=5 span_bits=17 shape=0 saved=0x1.dcp+8 off=77e27d058e817383 base=0e0a0a27a32b9948 planes=7613e7eadc45af4d
blocks_nnz257 col16 taken=1 mode=1 planes=0 words=6 span_bits=10 shape=0 saved=0x1.fap+8 off=924a081c073e4a2f base=7a59ee1096f08b5d planes=cbf29ce484222325
blocks_plane_nnz257 col16 taken=1 mode=1 planes=1 words=6 span_bits=17 shape=0 saved=0x1.d9ep+8 off=f0bc4243832ea8fb base=7a59ee1096f08b5d planes=cb632b8f348adaed
blocks_nnz513 col16 taken=1 mode=1 planes=0 words=10 span_bits=10 shape=0 saved=0x1.fbp+9 off=f76945d1fd88736e base=328c957878bb8579 planes=cbf29ce484222325
blocks_plane_nnz513 col16 taken=1 mode=1 planes=1 words=10 span_bits=17 shape=0 saved=0x1.dafp+9 off=4a2d2a44ff56aa57 base=328c957878bb8579 planes=2fb62b8d32e9b9a5
blocks_span65535 col16 taken=1 mode=1 planes=0 words=17 span_bits=16 shape=0 saved=0x1.fp+10 off=554bcefde48f2e44 base=6689c6d5f5c7468f planes=cbf29ce484222325
blocks_span65536 col16 taken=1 mode=1 planes=1 words=17 span_bits=17 shape=0 saved=0x1.d0cp+10 off=f55d1704d187cada base=6689c6d5f5c7468f planes=290f1e630f0b231c
blocks_2planes_auto col16 taken=0 span_bits=18
blocks_2planes_forced col16 taken=1 mode=1 planes=2 words=17 span_bits=18 shape=0 saved=0x1.b18p+10 off=3601a6f4bb0f566d base=6689c6d5f5c7468f planes=3a910ecfd843f745
blocks_8planes_forced col16 taken=1 mode=1 planes=8 words=17 span_bits=24 shape=0 saved=0x1.ecp+9 off=39593dee3e0d321b base=6689c6d5f5c7468f planes=65f1c21797d4f025
blocks_9planes_forced col16 taken=0 span_bits=25
blocks_no_col16 col16 taken=0 span_bits=10
blocks_no_col16_forced col16 taken=0 span_bits=10
blocks_resident_auto col16 taken=0 span_bits=0
blocks_resident_forced col16 taken=1 mode=1 planes=0 words=17 span_bits=10 shape=0 saved=0x1.fp+10 off=ebe0c62f825058ea base=6689c6d5f5c7468f planes=cbf29ce484222325
blocks_x120MB_f32 col16 taken=0 span_bits=0
blocks_x240MB_mixed col16 taken=1 mode=1 planes=0 words=17 span_bits=10 shape=0 saved=0x1.fp+10 off=ebe0c62f825058ea base=6689c6d5f5c7468f planes=cbf29ce484222325
blocks_split_row col16 taken=1 mode=1 planes=0 words=95 span_bits=13 shape=0 saved=0x1.d98p+10 off=02f87f8302a4bd30 base=333c514f8cd5d174 planes=cbf29ce484222325
blocks_no_nonzeros col16 taken=0 span_bits=0
groups_m1 col16 taken=1 mode=2 planes=0 words=0 span_bits=3 shape=2 saved=0x1.8p+2 off=63fcc5209ba9e8a9 base=ad6323825fa766dc planes=cbf29ce484222325
groups_m64 col16 taken=1 mode=2 planes=0 words=0 span_bits=8 shape=2 saved=0x1.3ep+9 off=8b03ffd36ef4f2e5 base=ad6323825fa766dc planes=cbf29ce484222325
groups_m65 col16 taken=1 mode=2 planes=0 words=0 span_bits=8 shape=2 saved=0x1.41p+9 off=2fe927e1bd5ea669 base=06262b6287ab8ac8 planes=cbf29ce484222325
groups_span65535 col16 taken=1 mode=2 planes=0 words=0 span_bits=16 shape=2 saved=0x1.e7p+10 off=fad28a461c129a83 base=b084897a6aa6f5f4 planes=cbf29ce484222325
groups_span65536 col16 taken=0 span_bits=0
groups_split_row col16 taken=1 mode=2 planes=0 words=0 span_bits=8 shape=2 saved=0x1.e6p+10 off=70bc48e8735a93ea base=22684c07ee414d2b planes=cbf29ce484222325
groups_split_row_nosplit col16 taken=0 span_bits=0
groups_empty_group col16 taken=1 mode=2 planes=0 words=0 span_bits=8 shape=2 saved=0x1.5p+10 off=f70ce7d5ec30b07d base=b76447dd2f169a5d planes=cbf29ce484222325
groups_tasks col16 taken=1 mode=2 planes=0 words=0 span_bits=8 shape=3 saved=0x1.e78p+10 off=929b724c3b871e4c base=64fed53106f0e8c7 planes=cbf29ce484222325
groups_tasks_split_row col16 taken=1 mode=2 planes=0 words=0 span_bits=8 shape=3 saved=0x1.e5p+10 off=ed0591cd2dcfc807 base=64fed53106f0e8c7 planes=cbf29ce484222325
groups_mode_off col16 taken=0 span_bits=0
groups_no_col16 col16 taken=0 span_bits=0
groups_wide_auto col16 taken=0 span_bits=0
groups_wide_mode1 col16 taken=1 mode=2 planes=0 words=0 span_bits=8 shape=2 saved=0x1.e88p+10 off=e98add9ca4a530b0 base=22684c07ee414d2b planes=cbf29ce484222325
groups_wide_flag col16 taken=1 mode=2 planes=0 words=0 span_bits=8 shape=2 saved=0x1.e88p+10 off=e98add9ca4a530b0 base=22684c07ee414d2b planes=cbf29ce484222325
groups_x120MB_f32 col16 taken=1 mode=2 planes=0 words=0 span_bits=8 shape=2 saved=0x1.e88p+10 off=e98add9ca4a530b0 base=22684c07ee414d2b planes=cbf29ce484222325
groups_x240MB_mixed col16 taken=0 span_bits=0
groups_no_tasks col16 taken=0 span_bits=0
slabs_b2_f64 xslabs B=2 saved=-0x1.778p+11 rp=daa525cfd36687f2 col=faa39807b61931de val=20912f502487245e
slabs_b3_f32 xslabs B=3 saved=-0x1.c3p+11 rp=2c6dd5c21c2e20d2 col=8de92b9ee71afa2e val=9805cbf89225e50e
slabs_b3_mixed xslabs B=3 saved=-0x1.778p+12 rp=2c6dd5c21c2e20d2 col=8de92b9ee71afa2e val=9805cbf89225e50e
slabs_b40_clipped xslabs B=32 saved=-0x1.6bc4p+16 rp=ab4ed36cbc004665 col=37bf02f96844458a val=3a0de257ec39f7a6
slabs_b1 xslabs B=0
slabs_off xslabs B=0
slabs_n_below_b xslabs B=2 saved=-0x1.94p+8 rp=4594f40da296696c col=08569d5ebf769ab4 val=76a74f2082c1ee45
slabs_n1 xslabs B=0
slabs_m1 xslabs B=2 saved=-0x1.8p+4 rp=b88f24ff2d1ce38c col=8560e6b70ace8465 val=10c4b223961b2de4
slabs_no_rows xslabs B=0
slabs_all_empty xslabs B=2 saved=-0x1.98p+7 rp=7479744ad77ee805 col=4d25767f9dce13f5 val=a8c7f832281a39c5
slabs_descending xslabs B=0
slabs_descending_in_slab xslabs B=2 saved=-0x1.778p+11 rp=8da4c50ce923928c col=b74f44c5a7bf0dbf val=530220ec0bf12225
slabs_split_row xslabs B=2 saved=-0x1.778p+11 rp=af47b01ab2ee4492 col=a0bac47487616aa6 val=39d7b71cde0df751
slabs_split_row_nosplit xslabs B=3 saved=-0x1.c3p+11 rp=218972ed8ec13b2b col=f731b8c32ff1c94a val=854f630a8d2cf96e
slabs_no_values xslabs B=0
slabs_vector_kernel xslabs B=0
slabs_auto_one_slab xslabs B=0
slabs_auto_resident xslabs B=0
slabs_auto_extra_cost xslabs B=0
split_4096 split n_long=0 n_chunks=0 long_nnz=0 long_t=4096 saved=0x1.fccp+12 long_row=cbf29ce484222325 long_cs=4d25767f9dce13f5 chunk_k=cbf29ce484222325
split_4097 split n_long=1 n_chunks=2 long_nnz=4097 long_t=4096 saved=-0x1.ap+5 long_row=ad2aca7747985764 long_cs=e8bd5042d485b2e7 chunk_k=959540a14cfd62c2
split_8192 split n_long=1 n_chunks=2 long_nnz=8192 long_t=4096 saved=-0x1p+7 long_row=4d25767f9dce13f5 long_cs=e8bd5042d485b2e7 chunk_k=fe0d57e12de08825
split_8193 split n_long=1 n_chunks=3 long_nnz=8193 long_t=4096 saved=-0x1p+7 long_row=ad2aca7747985764 long_cs=48c2a43a7e4ff656 chunk_k=4eeaf2106089be86
split_several split n_long=4 n_chunks=11 long_nnz=30386 long_t=4096 saved=0x1.df8p+12 long_row=235dad5dd5aa0847 long_cs=cf84ebf893678dc0 chunk_k=508921deb2bf6bd7
split_nosplit split n_long=0 n_chunks=0 long_nnz=0 long_t=2147483647 saved=0x1.0b5cp+16 long_row=cbf29ce484222325 long_cs=4d25767f9dce13f5 chunk_k=cbf29ce484222325
split_no_rows split n_long=0 n_chunks=0 long_nnz=0 long_t=4096 saved=0x0p+0 long_row=cbf29ce484222325 long_cs=4d25767f9dce13f5 chunk_k=cbf29ce484222325
rules_median rules serial_len=1 wants_csort=0
rules_no_serial_rows rules serial_len=0 wants_csort=0
rules_median_40 rules serial_len=40 wants_csort=0
rules_kernel_csort rules serial_len=4 wants_csort=1
rules_csort_on rules serial_len=4 wants_csort=1
rules_ordered rules serial_len=4 wants_csort=0
rules_serial rules serial_len=8 wants_csort=0
rules_mixed rules serial_len=8 wants_csort=0
rules_auto_scattered rules serial_len=8 wants_csort=1
rules_auto_reproducible rules serial_len=8 wants_csort=1
rules_auto_local rules serial_len=4 wants_csort=0
rules_auto_off rules serial_len=8 wants_csort=0
rules_auto_slabs_forced rules serial_len=8 wants_csort=0
rules_auto_stream_kernel rules serial_len=8 wants_csort=0
rules_auto_resident rules serial_len=8 wants_csort=0
saved_formulas csort=-0x1.d1f93cp+22 slices=0x1.7cbb4p+22 dict=0x1.27468p+22 group16=0x1.47b5ap+22 block16=0x1.07ffc1p+22 slabs=-0x1.e84cp+22 col32=0x0p+0
row_tables_check: 88 cases decoded
"""


def test_row_tables_round_trip_and_digests():
    p = subprocess.run([str(CHECK)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    got, want = p.stdout.splitlines(), EXPECTED.splitlines()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
