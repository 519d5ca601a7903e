"""graal_map_windows at mid-size shapes (tests/window_cases.m1 and m2, engines in the STEPPED state of tests/engine_states.engine_in):
11,000 and 8,997 ranks, 600,000 contacts (two grid passes of the streaming kernel), a bitmap of several hundred words, windows across
contig boundaries and a ring's wrap, pixels wider than a wave.  Grid-aligned windows are held to the crop of graal_layout_maps (pinned by
tests/test_maps_midsize_gpu.py); the others to tests/window_map_reference.windows_of, which prices only the window's own pairs
(sim_reference.sub_records + pair_lambda) with tests/test_maps_gpu.py's bound |E - E_ref| <= 1e-6 E_ref + terms 2^-30.

A pair that expects 2^31 contacts or more does not fit the maps' fixed point and makes its pixel NaN by design (graal_layout_maps does
the same): a pixel whose largest single lambda is within 1e-6 of 2^31 may be NaN, one above it must be, no other is."""
import numpy as np
import pytest

from tests import map_reference as MR
from tests import window_map_reference as WMR
from tests.engine_states import GRID_CONTACTS, cached, engine_in
from tests.test_maps_midsize_gpu import got as full_maps, problem

pytestmark = pytest.mark.gpu

# per case: (origins, px_rows, px_cols, bin) by key
M1 = {"aligned": ([[0, 0], [2400, 2700], [9900, 10050]], 300, 300, 3),
      "boundary": ([[2599 - 128, 2599 - 128]], 256, 256, 1),        # across the boundary of the two longest contigs (rank 2,599)
      "ring": ([[299, 799 - 256]], 256, 256, 1),                    # rows from the ring's first rank, columns up to its last: its wrap
      "diagonal": ([[5000, 5000]], 256, 256, 1),
      "far": ([[3000, 6000]], 256, 256, 1),                         # inside the long contig, 3,000 fragments (~450 kb) off the diagonal
      "wide": ([[17, 17]], 40, 40, 64)}
M2 = {"bin1": ([[1001, 1001], [3301, 3250], [8900, 8800]], 200, 200, 1),
      "bin4": ([[1001, 1003], [5, 2], [8801, 8902]], 60, 60, 4)}


def rendered(name):
    """{key: Engine.map_windows} of one stepped engine of the case, computed once and shared (read only)."""
    def make():
        P, s = problem(name)
        e, layout, _ = engine_in("stepped", P, layout=s)
        out = {}
        try:
            for key, args in (M1 if name == "m1" else M2).items():
                out[key] = e.map_windows(*args)
        finally:
            e.close()
        for v in out.values():
            for x in v[:4]:
                x.setflags(write=False)
        return out
    return cached(("windows got", name), make)


def reference(name, key):
    def make():
        P, s = problem(name)
        return WMR.windows_of(P, s, *(M1 if name == "m1" else M2)[key])
    return cached(("windows ref", name, key), make)


def check(label, got, W):
    obs, exp, res, rank, nbad = got
    assert np.array_equal(rank, W["rank_of_sub"]) and np.array_equal(obs, W["observed"]), label
    nan = np.isnan(exp)
    assert nbad == int(nan.sum()) and np.array_equal(nan, np.isnan(res)), label
    assert not np.any(nan & (W["largest"] < 2.0 ** 31 * (1 - 1e-6))) and np.all(nan[W["largest"] > 2.0 ** 31 * (1 + 1e-6)]), label
    err = np.abs(exp.astype(np.float64) - W["expected"])
    tol = 1e-6 * W["expected"] + W["terms"] * 2.0 ** -30
    with np.errstate(all="ignore"):
        ratio = float(np.nanmax(np.where(err > 0, err / tol, 0.0)))
    print("%s: largest |E - E_ref| / tolerance %.3f, %d NaN pixels" % (label, ratio, nbad))
    assert np.all((err <= tol) | nan), (label, ratio)
    o, ex, r = (x.astype(np.float64) for x in (obs, exp, res))
    ref = MR.residual(o, ex)
    rtol = 2.0 ** -22 * ((np.abs(o) + np.abs(ex)) / np.sqrt(np.where(ex > 0, ex, 1.0)) + np.abs(ref)) + 1e-30
    assert np.all((np.abs(r - ref) <= rtol) | nan), label
    return nan


def test_m1_engages():
    P, s = problem("m1")
    assert len(P["coo_row"]) > GRID_CONTACTS and int(P["init_n_sub_frags"]) == 11000          # two grid passes; 344 bitmap words
    order = MR.order_of(P["np_sub_frags_id"], s)
    label = np.zeros(len(order), dtype=np.int64)
    label[:] = s["id_c"][order]                                # (one sub-fragment per fragment: its id is the fragment's)
    starts = np.nonzero(np.diff(label))[0] + 1
    assert starts.tolist() == [36, 99, 299, 799, 2599]          # the contigs by ascending length: 36, 63, 200, 500 (the ring), 1,800, 8,401
    assert np.all(s["circ"][order[299:799]] == 1) and s["circ"].sum() == 500
    assert full_maps("m1", "stepped")[4096][4] == 3             # the full map's bin


def test_m1_aligned_windows_are_crops_of_the_full_map():
    O, E, Rs, pix, b, bad = full_maps("m1", "stepped")[4096]
    origins, pr, pc, bn = M1["aligned"]
    obs, exp, res, rank, nbad = rendered("m1")["aligned"]
    assert bn == b and np.array_equal(rank // b, pix)
    for w, (u0, v0) in enumerate(origins):
        sl = (slice(u0 // b, u0 // b + pr), slice(v0 // b, v0 // b + pc))
        assert O[sl].shape == (pr, pc)
        for got, want in ((obs[w], O[sl]), (exp[w], E[sl]), (res[w], Rs[sl])):
            assert np.array_equal(got, want, equal_nan=True), w      # (the same integers and maps.h's mp_pixel on both sides)
    assert nbad == int(np.isnan(exp).sum()) and obs.sum() > 0 and np.nanmax(exp) > 0


@pytest.mark.parametrize("key", ["boundary", "ring", "diagonal"])
def test_m1_bin_1_windows(key):
    W = reference("m1", key)
    nan = check("m1 " + key, rendered("m1")[key], W)
    assert (W["cis"] & ~nan).sum() > 1000                       # cis-priced pixels: the comparison would notice a lost one
    if key == "boundary":
        cis = W["cis"][0]
        assert not cis[:128, 128:].any() and not cis[128:, :128].any() and cis[:128, :128].any() and cis[128:, 128:].any()
    if key == "ring":
        assert W["cis"].sum() == 256 * 256 - 12               # every pair is the ring's; ranks 543 .. 554 meet themselves on 12 pixels


def test_m1_beyond_the_window_is_the_background_exactly():
    P, s = problem("m1")
    W = reference("m1", "far")
    obs, exp, res, rank, nbad = rendered("m1")["far"]
    check("m1 far", rendered("m1")["far"], W)
    assert not W["cis"].any() and nbad == 0
    acc = np.asarray(P["np_sub_frags_accu"], dtype=np.int64).reshape(-1, 3)[:, 0][W["order"]]      # per rank (one sub-fragment per fragment)
    v = max(float(np.float32(P["param_simu"][7])), 0.0) / float(np.float32(P["mean_squared_frags_per_bin"]))
    want = (v * (acc[3000:3256, None] * acc[None, 6000:6256]).astype(np.float64)).astype(np.float32)
    assert np.array_equal(exp[0], want) and want.min() > 0


def test_m1_pixels_wider_than_a_wave():
    W = reference("m1", "wide")
    nan = check("m1 wide", rendered("m1")["wide"], W)
    assert (W["cis"] & ~nan).sum() > 100 and (W["terms"] == 64 * 64).any() and (W["terms"] == 64 * 63).sum() == 40


@pytest.mark.parametrize("key", ["bin1", "bin4"])
def test_m2_windows(key):
    P, s = problem("m2")
    sid = np.asarray(P["np_sub_frags_id"]).reshape(-1, 4)
    assert (sid[:, 3] == 3).sum() > 2900 and (s["ori"] == -1).sum() >= 700
    origins, pr, pc, b = M2[key]
    assert all(u % 3 and v % 3 and u % 4 and v % 4 for u, v in origins[:2])
    W = reference("m2", key)
    nan = check("m2 " + key, rendered("m2")[key], W)
    assert (W["cis"] & ~nan).sum() > 1000 and (W["terms"] == 0).any()          # (the last window of each set reaches past S)
