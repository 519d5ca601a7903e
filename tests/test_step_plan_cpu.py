"""CPU: the shape of a step (graal_amd/csrc/step_plan.h, compiled for the host into the test-only library): the producer and its grid,
bitmap and completion increments, the flow, the finisher, k_fin's grid, the tiled reference-arithmetic kernels' sizes and the full
evaluation's kernels.  Every expected value is a literal worked out by hand from the expressions the launchers held before the header
existed; each branch boundary is taken on both sides."""
import ctypes

import numpy as np

from tests import util

_i64p = ctypes.POINTER(ctypes.c_int64)

FIELDS = ("n n_sub_total nnz single_sub n_contigs max_lcont lcont_bound has_rep has_ubins uniform_accu strict quirk "
          "K world exchange publish ev finisher_ok spin_ok gwait_env mid_run has_rowptr longest_row forced_producer "
          "slist_soft_cap slist_floor slist_cap "
          "scan_threads scan_groups scan_blocks scan_fold_bits scan_rows_r fin_blocks strict_dense no_flat full_no_compact full_no_lds "
          "full_mass_tiled stage_tables lds_tm lds_fin regs_tm regs_fin fin_dyn_lds_per_k").split()

# the benchmark's exploded layout on one rank, synchronous path, every switch unset; k_fin's dynamic LDS is 3,700 bytes per neighbour
# (315 sums of 8 bytes + 295 ints), the kernels' figures chosen so that registers allow 4 blocks of k_fin next to k_tm and LDS 3 (K = 5)
BASE = dict(n=50000, n_sub_total=50000, nnz=20_000_000, single_sub=1, n_contigs=10000, max_lcont=5, lcont_bound=12, has_rep=0, has_ubins=0,
            uniform_accu=1, strict=0, quirk=0, K=5, world=1, exchange=0, publish=1, ev=0, finisher_ok=1, spin_ok=1, gwait_env=1, mid_run=0,
            has_rowptr=0, longest_row=0, forced_producer=0, slist_soft_cap=1 << 23, slist_floor=0, slist_cap=0,
            scan_threads=0, scan_groups=4, scan_blocks=496, scan_fold_bits=0, scan_rows_r=16, fin_blocks=0, strict_dense=0, no_flat=0,
            full_no_compact=0, full_no_lds=0, full_mass_tiled=-1, stage_tables=-1,
            lds_tm=43792, lds_fin=17808, regs_tm=96, regs_fin=96, fin_dyn_lds_per_k=3700)
NONE, KFIN, FLAT, TILED = 0, 1, 2, 3


def hc():
    L = util.hostcheck()
    for name in ("hc_plan_producer", "hc_plan_fin", "hc_plan_strict", "hc_plan_full"):
        getattr(L, name).restype = None
        getattr(L, name).argtypes = [_i64p, _i64p]
    L.hc_plan_flow.restype = None
    L.hc_plan_flow.argtypes = [_i64p, ctypes.c_int, _i64p]
    L.hc_plan_finisher.restype = ctypes.c_int
    L.hc_plan_finisher.argtypes = [_i64p, ctypes.c_int]
    L.hc_plan_n_facts.restype = ctypes.c_int
    assert L.hc_plan_n_facts() == len(FIELDS) == len(BASE)
    return L


def facts(**kw):
    assert not set(kw) - set(BASE), set(kw) - set(BASE)
    d = dict(BASE, **kw)
    return np.array([d[k] for k in FIELDS], np.int64)


def call(name, n_out, keys, *extra, **kw):
    f, out = facts(**kw), np.full(n_out, -7, np.int64)
    getattr(hc(), name)(f.ctypes.data_as(_i64p), *extra, out.ctypes.data_as(_i64p))
    return dict(zip(keys, out.tolist())), out


def producer(**kw):
    d, out = call("hc_plan_producer", 24, ("indexed", "impossible", "threads", "groups", "grid", "bitmap", "mask", "rows"), **kw)
    d["inc"] = out[8:].tolist()
    return d


def flow(indexed=0, **kw):
    return call("hc_plan_flow", 8, ("late_stage", "mid", "inline_m", "stage", "tm_publishes", "ticks", "rep_delta", "finisher"), indexed, **kw)[0]


def finisher(flat_first, **kw):
    return hc().hc_plan_finisher(facts(**kw).ctypes.data_as(_i64p), flat_first)


def fin(**kw):
    return call("hc_plan_fin", 3, ("grid", "event", "no_wait"), **kw)[0]


def strict(**kw):
    return call("hc_plan_strict", 13, ("dense", "grid", "tile", "nt", "refused", "seg_unit", "target", "worst", "need", "alloc", "gwait",
                                       "cull_blocks", "no_window"), **kw)[0]


def full(**kw):
    return call("hc_plan_full", 7, ("compact", "nnz_kernel", "nnz_grid", "lab_bytes", "mass_kernel", "mass_grid", "S"), **kw)[0]


ALL_ONES = 0xffffffff


# ---- the producer
def test_streaming_threads_and_grid():
    p = producer()                                   # 5,000,001 groups of 4, 4 x 1,024 per block and iteration: 1,221 blocks wanted, 496 given
    assert (p["indexed"], p["threads"], p["groups"], p["grid"]) == (0, 1024, 4, 496)
    p = producer(nnz=900)
    assert (p["threads"], p["grid"]) == (256, 1)
    p = producer(nnz=0)
    assert (p["threads"], p["grid"]) == (256, 1)
    p = producer(nnz=1_999_999)                      # 500,000 groups / (4 x 256) = 488.3
    assert (p["threads"], p["grid"]) == (256, 489)
    p = producer(nnz=2_000_000)                      # 500,001 groups / (4 x 1,024) = 122.1
    assert (p["threads"], p["grid"]) == (1024, 123)
    p = producer(scan_threads=512)                   # the switch: 5,000,001 / 2,048 = 2,441.4
    assert (p["threads"], p["grid"]) == (512, 496)
    p = producer(nnz=1_000_000, scan_threads=512)    # 250,001 / 2,048 = 122.07
    assert (p["threads"], p["grid"]) == (512, 123)
    p = producer(scan_groups=8, scan_blocks=248)     # 5,000,001 / 8,192 = 610.4
    assert (p["groups"], p["grid"]) == (8, 248)
    p = producer(nnz=160_000)                        # 40,001 / 1,024 = 39.06
    assert (p["threads"], p["grid"]) == (256, 40)


def test_bitmap_and_its_fold():
    p = producer(n_sub_total=50_000)                 # 1,563 words + 2
    assert (p["bitmap"], p["mask"]) == (6260, ALL_ONES)
    p = producer(n_sub_total=400_000)                # 50,008 bytes > 49,152: folded onto 2^18 bits = 8,192 words
    assert (p["bitmap"], p["mask"]) == (32768, 8191)
    # the boundary is where (words + 2) * 4 > 49,152 puts it: 12,286 words still fit, i.e. 393,152 ids (not the round 393,216)
    p = producer(n_sub_total=393_152)
    assert (p["bitmap"], p["mask"]) == (49152, ALL_ONES)
    p = producer(n_sub_total=393_153)
    assert (p["bitmap"], p["mask"]) == (32768, 8191)
    # the switch folds whatever the size -- unless 2^b bits hold every id
    p = producer(n_sub_total=50_000, scan_fold_bits=10)
    assert (p["bitmap"], p["mask"]) == (128, 31)
    p = producer(n_sub_total=1024, scan_fold_bits=10)     # 32 words + 2
    assert (p["bitmap"], p["mask"]) == (136, ALL_ONES)
    p = producer(n_sub_total=1025, scan_fold_bits=10)
    assert (p["bitmap"], p["mask"]) == (128, 31)


def test_indexed_or_streaming():
    idx = dict(has_rowptr=1, longest_row=557)
    p = producer(**idx)                              # 6 contigs x 12 fragments = 72 rows; 72 x 557 x 16 = 641,664 <= 20 M; 75 / 4 = 18 blocks
    assert (p["indexed"], p["impossible"], p["rows"], p["grid"]) == (1, 0, 72, 18)
    assert p["inc"] == [2, 2] + [1] * 14
    assert (p["threads"], p["groups"]) == (1024, 4)  # (the streaming pass's figures, whatever the producer)
    assert producer(ev=1, **idx)["indexed"] == 0 and producer(ev=1, **idx)["grid"] == 496      # an event pair: streams
    assert producer(forced_producer=1, **idx)["indexed"] == 0
    assert producer(longest_row=557)["indexed"] == 0                                           # no index
    assert producer(n_sub_total=400_000, **idx)["indexed"] == 0                                # folded bitmap
    # the switch, on both sides: 2 contigs x 50 = 100 rows, longest row 100, R = 16
    sw = dict(K=1, max_lcont=50, lcont_bound=0, has_rowptr=1, longest_row=100)
    p = producer(nnz=160_000, **sw)
    assert (p["indexed"], p["rows"], p["grid"]) == (1, 100, 25)
    p = producer(nnz=159_999, **sw)
    assert (p["indexed"], p["grid"]) == (0, 40)
    assert producer(nnz=159_999, scan_rows_r=15, **sw)["indexed"] == 1
    # the rows the pass's list holds: 2,048.  K = 5, one sub-fragment per bin: 6 x 341 = 2,046, 6 x 342 = 2,052; the grid stops at 64
    p = producer(max_lcont=341, lcont_bound=0, has_rowptr=1, longest_row=1)
    assert (p["indexed"], p["rows"], p["grid"]) == (1, 2046, 64)
    assert producer(max_lcont=342, lcont_bound=0, has_rowptr=1, longest_row=1)["indexed"] == 0
    # three sub-fragments per bin: 6 x 113 x 3 = 2,034, 6 x 114 x 3 = 2,052; the bound is the larger of the two lengths
    assert producer(single_sub=0, max_lcont=5, lcont_bound=113, has_rowptr=1, longest_row=1)["rows"] == 2034
    assert producer(single_sub=0, max_lcont=5, lcont_bound=113, has_rowptr=1, longest_row=1)["indexed"] == 1
    assert producer(single_sub=0, max_lcont=114, lcont_bound=12, has_rowptr=1, longest_row=1)["indexed"] == 0


def test_forced_indexed_pass():
    p = producer(forced_producer=2, has_rowptr=1, longest_row=10 ** 6)     # forced: indexed although it would lose
    assert (p["indexed"], p["impossible"], p["grid"]) == (1, 0, 18)
    p = producer(forced_producer=2, has_rowptr=1, longest_row=557, ev=1)   # ... and although the call carries an event pair
    assert (p["indexed"], p["impossible"]) == (1, 0)
    for kw in (dict(has_rowptr=0), dict(has_rowptr=1, n_sub_total=400_000), dict(has_rowptr=1, max_lcont=342, lcont_bound=0)):
        p = producer(forced_producer=2, **kw)
        assert (p["indexed"], p["impossible"]) == (0, 1), kw
    assert producer(forced_producer=0, has_rowptr=0)["impossible"] == 0   # not forced: nothing to report


def test_completion_increments_sum_to_the_grid():
    for g in range(1, 4097):
        p = producer(nnz=4_000_000_000, scan_blocks=g)
        assert p["grid"] == g and sum(p["inc"]) == g and max(p["inc"]) - min(p["inc"]) <= 1
    for lc in range(1, 342, 7):                      # and of the indexed pass's grids
        p = producer(max_lcont=lc, lcont_bound=0, forced_producer=2, has_rowptr=1)
        assert p["grid"] == min((6 * lc + 3) // 4, 64) and sum(p["inc"]) == p["grid"]


# ---- the flow
def test_flow_of_the_default_arithmetic():
    f = flow()
    assert f == dict(late_stage=0, mid=0, inline_m=20, stage=1, tm_publishes=1, ticks=21000, rep_delta=0, finisher=NONE)
    assert flow(indexed=1)["stage"] == 0             # the indexed pass is a short scan
    assert flow(nnz=3_999_999)["stage"] == 0 and flow(nnz=4_000_000)["stage"] == 1
    assert flow(stage_tables=0)["stage"] == 0 and flow(indexed=1, nnz=900, stage_tables=1)["stage"] == 1
    assert flow(nnz=0)["ticks"] == 5000 and flow(nnz=900)["ticks"] == 5000 and flow(nnz=2 * 10 ** 15)["ticks"] == 1 << 30
    for kw in (dict(publish=0), dict(finisher_ok=0), dict(world=2), dict(has_rep=1)):
        f = flow(**kw)
        assert (f["tm_publishes"], f["finisher"], f["rep_delta"]) == (0, KFIN, kw.get("has_rep", 0)), kw
    assert flow(world=2, exchange=1)["tm_publishes"] == 1


def test_late_stage():
    late = dict(n=520, n_contigs=2)
    assert flow(max_lcont=128, **late)["late_stage"] == 0 and flow(max_lcont=129, **late)["late_stage"] == 1
    assert flow(max_lcont=200, n_contigs=8, n=512)["late_stage"] == 0 and flow(max_lcont=200, n_contigs=8, n=513)["late_stage"] == 1
    f = flow(max_lcont=260, **late)
    assert (f["tm_publishes"], f["finisher"]) == (0, KFIN)
    f = flow(max_lcont=260, strict=1, mid_run=1, **late)                  # reference arithmetic: the tiled kernels, no flat kernel, not `mid`
    assert (f["mid"], f["inline_m"], f["tm_publishes"], f["finisher"]) == (0, 20, 0, TILED)
    f = flow(max_lcont=260, strict=1, world=2, exchange=1, **late)
    assert f["finisher"] == TILED


def test_flow_of_the_reference_arithmetic():
    f = flow(strict=1)
    assert (f["mid"], f["inline_m"], f["tm_publishes"], f["finisher"]) == (0, 20, 1, NONE)
    f = flow(strict=1, mid_run=1)
    assert (f["mid"], f["inline_m"], f["tm_publishes"], f["finisher"]) == (1, 0, 0, FLAT)
    for kw in (dict(no_flat=1), dict(world=2, exchange=1)):               # `mid` is one rank's flow, and needs the flat kernel
        f = flow(strict=1, mid_run=1, **kw)
        assert (f["mid"], f["inline_m"], f["tm_publishes"], f["finisher"]) == (0, 20, 1, NONE), kw
    f = flow(strict=1, mid_run=1, finisher_ok=0)
    assert (f["mid"], f["tm_publishes"], f["finisher"]) == (0, 0, TILED)
    f = flow(strict=1, mid_run=1, publish=0)                              # the asynchronous path
    assert (f["mid"], f["tm_publishes"], f["finisher"]) == (0, 0, TILED)
    f = flow(strict=1, mid_run=1, strict_dense=1)
    assert (f["mid"], f["inline_m"], f["tm_publishes"], f["finisher"]) == (0, -1, 0, TILED)
    assert flow(strict=0, strict_dense=1)["tm_publishes"] == 1 and flow(strict=0, strict_dense=1)["inline_m"] == -1
    f = flow(strict=1, has_rep=1)
    assert (f["rep_delta"], f["tm_publishes"], f["finisher"]) == (1, 0, TILED)
    # several ranks: whoever finishes a step outside the late stage goes through the flat kernel first
    f = flow(strict=1, world=2, exchange=1, finisher_ok=0)
    assert (f["tm_publishes"], f["finisher"]) == (0, FLAT)
    f = flow(strict=1, world=2, exchange=0, publish=0)                    # a communicator: nothing is handed back through the host
    assert (f["tm_publishes"], f["finisher"]) == (0, TILED)


def test_the_rule_for_a_step_handed_back():
    assert finisher(1) == KFIN and finisher(0) == KFIN
    assert finisher(1, strict=1) == FLAT and finisher(0, strict=1) == TILED       # one try of the flat kernel
    for kw in (dict(no_flat=1), dict(strict_dense=1), dict(publish=0), dict(world=2)):
        assert finisher(1, strict=1, **kw) == TILED, kw
    assert finisher(1, strict=1, world=2, exchange=1) == FLAT


# ---- k_fin
def test_grid_of_k_fin():
    # room next to k_tm: LDS (163,840 - 43,792) / (17,808 + 5 x 3,700) = 3.3, registers (512 - 96) / 96 = 4.3: 3 blocks per CU
    assert fin(max_lcont=16) == dict(grid=32, event=0, no_wait=768)
    assert fin(max_lcont=17) == dict(grid=768, event=0, no_wait=768)
    assert fin(max_lcont=0) == dict(grid=768, event=0, no_wait=768)       # (no statistics yet)
    assert fin(max_lcont=1024) == dict(grid=768, event=0, no_wait=768)
    assert fin(max_lcont=1025) == dict(grid=2048, event=1, no_wait=768)
    assert fin(max_lcont=300, K=10) == dict(grid=512, event=0, no_wait=512)   # LDS: 120,048 / 54,808 = 2.2
    assert fin(max_lcont=300, regs_tm=137, regs_fin=137) == dict(grid=512, event=0, no_wait=512)   # registers: (512 - 144) / 144 = 2.6
    # what the runtime does not report: 64 KB, 32 KB, 128, 128 -- LDS 98,304 / 51,268 = 1.9
    assert fin(max_lcont=300, lds_tm=65536, lds_fin=32768, regs_tm=128, regs_fin=128) == dict(grid=256, event=0, no_wait=256)
    assert fin(max_lcont=300, lds_tm=200000) == dict(grid=256, event=0, no_wait=256)               # never fewer than one block per CU
    assert fin(max_lcont=5, fin_blocks=768) == dict(grid=768, event=0, no_wait=768)                # the switch
    assert fin(max_lcont=5, fin_blocks=769) == dict(grid=769, event=1, no_wait=768)


# ---- the tiled reference-arithmetic kernels
S = dict(n=2000, strict=1, max_lcont=100, lcont_bound=202)


def test_strict_grid_tile_and_entries():
    assert [strict(**dict(S, max_lcont=m))["grid"] for m in (0, 64, 65, 256, 257)] == [32, 32, 512, 512, 1024]
    assert [strict(**dict(S, max_lcont=m))["target"] for m in (64, 65, 257)] == [768, 12288, 24576]
    assert strict(**dict(S, max_lcont=64, lcont_bound=130))["grid"] == 32          # the grid by the longest contig as last seen, not its bound
    assert strict(**S)["tile"] == 64 and strict(single_sub=0, **S)["tile"] == 32
    assert [strict(**dict(S, max_lcont=m, lcont_bound=0))["seg_unit"] for m in (512, 513)] == [4, 16]
    assert [strict(single_sub=0, **dict(S, max_lcont=m, lcont_bound=0))["seg_unit"] for m in (512, 513)] == [2, 4]
    assert strict(**dict(S, max_lcont=200, lcont_bound=513))["seg_unit"] == 16     # ... by the bound
    assert strict(**S)["no_window"] == 0 and strict(quirk=1, **S)["no_window"] == 0 and strict(has_ubins=1, **S)["no_window"] == 0
    assert strict(quirk=1, has_ubins=1, **S)["no_window"] == 1
    d = strict(strict_dense=1, **S)
    assert d["dense"] == 1 and d["grid"] == 0 and d["refused"] == 0


def test_strict_tiles_and_their_refusal():
    # 6 contigs x ceil(602 / 64) = 60 tiles, or every fragment: 32 tiles + 6; + 33 global pieces
    p = strict(**dict(S, max_lcont=300, lcont_bound=602))
    assert (p["nt"], p["refused"], p["cull_blocks"]) == (38 + 33, 0, 71)
    p = strict(**dict(S, n=10 ** 6, max_lcont=300, lcont_bound=602))
    assert (p["nt"], p["cull_blocks"]) == (60 + 33, 93)
    p = strict(single_sub=0, **dict(S, n=10 ** 6))       # tiles of 32: 6 x ceil(202 / 32) = 42
    assert p["nt"] == 42 + 33
    # 65,536 tiles and more are refused.  By the fragments, K = 10: ceil(n / 64) + 11 + 33
    big = dict(strict=1, K=10, max_lcont=4_200_000, lcont_bound=0)
    p = strict(n=4_191_361, **big)
    assert (p["nt"], p["refused"], p["cull_blocks"]) == (65535, 0, 1024)
    p = strict(n=4_191_425, **big)
    assert (p["nt"], p["refused"]) == (65536, 1)
    # by the contigs: 11 x ceil(lc / 64) + 33
    p = strict(n=4_200_000, **dict(big, max_lcont=381_056))
    assert (p["nt"], p["refused"]) == (11 * 5954 + 33, 0)
    p = strict(n=4_200_000, **dict(big, max_lcont=381_057))
    assert (p["nt"], p["refused"]) == (11 * 5955 + 33, 1)


def test_strict_list_sizes():
    # the largest union: 32 tiles + 11 + 33 = 76, 76 x 77 / 2 = 2,926 tile pairs, 64 / 4 entries each, + 64
    p = strict(**S)
    assert (p["worst"], p["need"], p["alloc"]) == (46880, 46880, 46880)
    p = strict(**dict(S, max_lcont=300, lcont_bound=602))                 # entries of 16 fragments
    assert (p["worst"], p["need"]) == (2926 * 4 + 64, 11768)
    p = strict(single_sub=0, **S)                                          # tiles of 32: 63 + 44 = 107, 5,778 pairs, 16 entries each
    assert p["worst"] == 92512
    assert strict(slist_cap=46880, **S)["alloc"] == 0 and strict(slist_cap=46879, **S)["alloc"] == 46880
    # one rank: the soft cap, the floor a grown list raised, never more than the worst case
    assert strict(slist_soft_cap=1000, **S)["need"] == 1000
    assert strict(slist_soft_cap=1000, slist_floor=5000, **S)["need"] == 5000
    assert strict(slist_soft_cap=1000, slist_floor=10 ** 6, **S)["need"] == 46880
    p = strict(slist_soft_cap=1000, slist_cap=1000, **S)
    assert (p["need"], p["alloc"]) == (1000, 0)
    p = strict(slist_soft_cap=10, **S)                                     # 64 entries at least
    assert (p["need"], p["alloc"]) == (10, 64)
    assert strict(slist_soft_cap=10, slist_cap=10, **S)["alloc"] == 0
    # several ranks, or a step that does not publish to the host: the worst case
    assert strict(slist_soft_cap=1000, world=2, **S)["need"] == 46880
    assert strict(slist_soft_cap=1000, publish=0, **S)["need"] == 46880


def test_hand_off_behind_k_gprep():
    assert strict(**S)["gwait"] == 1
    for kw in (dict(gwait_env=0), dict(publish=0), dict(world=2), dict(spin_ok=0), dict(max_lcont=257)):
        assert strict(**dict(S, **kw))["gwait"] == 0, kw
    assert strict(**dict(S, max_lcont=256))["gwait"] == 1 and strict(**dict(S, max_lcont=10))["gwait"] == 1


# ---- the full evaluation
def test_full_evaluation_kernels():
    NNZ_NONE, NNZ_PLAIN, NNZ_U, NNZ_L = 0, 1, 2, 3
    M64, M16, MT = 0, 1, 2
    p = full()                                       # labels in LDS: 100,000 bytes; 5,000,001 groups / 2,048 = 2,441.4 -> 256 blocks
    assert p == dict(compact=1, nnz_kernel=NNZ_L, nnz_grid=256, lab_bytes=100000, mass_kernel=M16, mass_grid=3125, S=0)
    p = full(nnz=2_000_000)                          # 500,001 / 2,048 = 244.1
    assert (p["nnz_kernel"], p["nnz_grid"]) == (NNZ_L, 245)
    p = full(nnz=1_999_999)                          # 500,000 / 512 = 976.6
    assert (p["nnz_kernel"], p["nnz_grid"]) == (NNZ_U, 977)
    p = full(n_sub_total=76_800)
    assert (p["nnz_kernel"], p["lab_bytes"]) == (NNZ_L, 153600)
    p = full(n_sub_total=76_801)                     # 5,000,001 / 512 = 9,765.6 -> 2,048 blocks
    assert (p["nnz_kernel"], p["lab_bytes"], p["nnz_grid"]) == (NNZ_U, 153616, 2048)
    assert full(full_no_lds=1)["nnz_kernel"] == NNZ_U
    p = full(full_no_compact=1)
    assert (p["compact"], p["nnz_kernel"], p["nnz_grid"]) == (0, NNZ_PLAIN, 2048)
    assert full(uniform_accu=0)["nnz_kernel"] == NNZ_PLAIN and full(uniform_accu=0)["compact"] == 0
    p = full(nnz=0)
    assert (p["compact"], p["nnz_kernel"], p["nnz_grid"], p["lab_bytes"]) == (1, NNZ_NONE, 0, 0)
    # the mass kernels
    p = full(n=16384)
    assert (p["mass_kernel"], p["mass_grid"]) == (M64, 4096)
    p = full(n=16385)
    assert (p["mass_kernel"], p["mass_grid"]) == (M16, 1025)
    p = full(max_lcont=256, lcont_bound=0)
    assert p["mass_kernel"] == M16
    p = full(max_lcont=257, lcont_bound=0)           # 782 tiles; ceil(257 / 64) = 5 tiles of a contig: one wave per x tile
    assert (p["mass_kernel"], p["S"], p["mass_grid"]) == (MT, 1, 196)
    p = full(max_lcont=100, lcont_bound=7000)        # (110 + 7) / 8 = 14 waves per x tile; (782 x 14 + 3) / 4
    assert (p["mass_kernel"], p["S"], p["mass_grid"]) == (MT, 14, 2737)
    p = full(max_lcont=60000, lcont_bound=0)         # no longer than the map: (782 + 7) / 8 = 98 -> 16
    assert (p["S"], p["mass_grid"]) == (16, 3128)
    assert full(n=16384, max_lcont=7000)["mass_kernel"] == M64            # a small map keeps one wave per fragment
    assert full(max_lcont=7000, full_mass_tiled=0)["mass_kernel"] == M16
    p = full(n=1000, full_mass_tiled=1)              # 16 tiles, one wave each
    assert (p["mass_kernel"], p["S"], p["mass_grid"]) == (MT, 1, 4)
