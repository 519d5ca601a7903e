"""graal_layout_maps at mid-size shapes, against the numpy restatement (tests/map_reference.py) with the chunked brute force over every
sub-fragment pair (map_reference.expected_chunked) as the expected image.  tests/test_maps_gpu.py's largest case has 240 slots: one block
of k_mp_cis, one grid pass of k_mp_obs, pixels narrower than a wave, and an engine that never stepped.

Engine states (tests/engine_states.engine_in).  k_mp_cis lets Sw waves share a 64-slot x tile; the handle takes Sw from
the longest contig of its last graal_begin_step, which an upload leaves alone.  Every claim below about several waves per tile, a wave's
second chunk and waves that leave at once holds for the STEPPED state (upload, then begin_step: what every run does before it draws a map)
and for the STALE one; on a FRESH engine (upload only) Sw is 1 whatever the layout, and what the shapes reach there is the number of
tiles, blocks and grid passes and the pixel widths.  Every case's layout is the relabelled one (contigs by ascending length, as begin_step
leaves them), so the fresh and the stepped engine hold the same layout and one reference serves both.

Cases (stepped Sw in brackets):
  m1        [16] 11,000 slots of one sub-fragment, contigs of 8,401 / 1,800 / 500 (a ring) / 200 / 63 / 36, 600,000 contacts (two grid
            passes of k_mp_obs), a window of ~1,550 slots > 64 * 16: the cap of 16 limits Sw and a wave takes a second chunk.  max_px 4096
            (bin 3: 3,667^2 pixels that straddle wave and tile boundaries), 100 (bin 110: wider than a wave) and 7;
  m1_narrow [16] the same layout with a 12 kb window of at most 114 slots, so that a tile's pairs end within its first three chunks:
            waves 3 .. 15 of a tile stage one chunk, find it beyond the window and leave.  max_px 100.  (m1's 25 kb variant, which the
            links tests use, has windows of up to 214 slots: too wide for that.);
  m2        [3]  3,000 slots of up to 3 sub-fragments, RF counts 1 .. 4, every 4th bin reversed, 8,997 sub-fragments.  max_px 4096 (bin 3:
            ranks not aligned with slots) and 50;
  m3        [3]  3,000 slots of one sub-fragment, contigs of 1,500 / 900 / 400 (a ring) / 200, a window of ~240 slots.  max_px 4096: bin 1,
            no run merging, every term its own atomic;
  m1_cut    STALE [16 on contigs of at most 500 slots]: begin_step on m1's layout, then upload of m1_cut's.  max_px 100.

Every test asserts that its shape engages, and that the comparison would notice a lost tile: what the brute force adds for cis pairs at
least 64 slots apart (behind a wave's first staged chunk whatever its lane) -- and on m1 at least 64 * Sw slots apart (a wave's second
chunk) -- exceeds the tolerance in 36 pixels or more.  (Not asserted of m1's 7 x 7 image: the window reaches its 19 pixels on and
next to the diagonal and no more; the same launches are held to it at 3,667 and 100 pixels a side.)"""
import time

import numpy as np
import pytest

from graal_amd.lib import Q_SCALE
from tests import map_reference as MR
from tests import window_cases as WC
from tests import window_reference as WR
from tests.engine_states import GRID_CONTACTS, cached, engine_in, relabelled, stripes_of

pytestmark = pytest.mark.gpu

#        name: (problem, max_px list, stepped Sw, bin per max_px)
CASES = {"m1": (WC.m1, (4096, 100, 7), 16, (3, 110, 1572)),
         "m1_narrow": (lambda: WC.m1(d_max=12.0), (100,), 16, (110,)),
         "m2": (WC.m2, (4096, 50), 3, (3, 180)),
         "m3": (WC.m3, (4096,), 3, (1,)),
         "m1_cut": (WC.m1_cut, (100,), 1, (110,))}
STEPPED = [(name, px) for name in ("m1", "m1_narrow", "m2", "m3") for px in CASES[name][1]]
FAR = 64                                 # slots: a pair this far apart lies behind the first chunk its x wave stages


def problem(name):
    """(P, the relabelled layout every engine of the case is given)"""
    def make():
        P = CASES[name][0]()
        s = relabelled(P["S_o_A_frags"])
        for v in s.values():
            v.setflags(write=False)
        return P, s
    return cached(("maps", name), make)


def reference(name):
    """{max_px: order, pixel_of_sub, bin, m, observed, expected, tol, far} of a case, computed once and shared (read only)."""
    def make():
        t0 = time.time()
        P, s = problem(name)
        far = (FAR, 64 * 16) if name == "m1" else (FAR,)
        out = MR.expected_chunked(P, s, CASES[name][1], far)
        for px, R in out.items():
            order, pix, b, m = MR.pixels(P["np_sub_frags_id"], s, px)
            assert (b, m) == (R["bin"], R["m"])
            R.update(order=order, pixel_of_sub=pix, observed=MR.observed(P["coo_row"], P["coo_col"], P["coo_val"], pix, m))
            R["tol"] = 1e-6 * R["expected"] + R.pop("terms") * 2.0 ** -30
            R["far"] = {d: int((np.abs(F) > R["tol"]).sum()) for d, F in R["far"].items()}      # (pixels it moves by more than the tolerance)
            for x in [R[k] for k in ("pixel_of_sub", "observed", "expected", "tol")]:
                x.setflags(write=False)
        print("%s: reference in %.1f s" % (name, time.time() - t0))
        return out
    return cached(("maps ref", name), make)


def got(name, engine_state):
    """{max_px: Engine.layout_maps, "again": a second call at the first max_px behind the others, "mass": the full evaluation's expected
    mass, "Sw"} of one engine of the case in that state, computed once and shared (read only)."""
    def make():
        P, s = problem(name)
        before = problem("m1")[1] if engine_state == "stale" else None
        e, layout, Sw = engine_in(engine_state, P, layout=s, before=before)
        out = {"Sw": Sw}
        try:
            for k in layout:      # (the relabel of a relabelled layout changes nothing: the reference's layout is the engine's)
                assert np.array_equal(layout[k], s[k]), k
            pxs = CASES[name][1]
            t0 = time.time()
            for px in pxs:
                out[px] = e.layout_maps(px)
            if len(pxs) > 1:
                out["again"] = e.layout_maps(pxs[0])
            out["seconds"] = time.time() - t0
            e.relabel_contigs()
            out["mass"] = -float(int(e.eval_full_q()[1])) / Q_SCALE
        finally:
            e.close()
        for px in pxs + (("again",) if len(pxs) > 1 else ()):
            for x in out[px][:4]:
                x.setflags(write=False)
        return out
    return cached(("maps got", name, engine_state), make)


def window_slots(s, d_max_kb):
    """The most slots y behind a slot x of a linear contig that k_mp_cis prices: start(y) - end(x) <= reach_bp."""
    reach = WR.reach_bp(float(np.float32(d_max_kb)))
    widest = 0
    for c in np.unique(s["id_c"]):
        mem = np.nonzero((s["id_c"] == c) & (s["circ"] == 0))[0]
        if len(mem) < 2:
            continue
        mem = mem[np.argsort(s["pos"][mem])]
        start = s["start_bp"][mem].astype(np.int64)
        last = np.searchsorted(start, start + s["len_bp"][mem] + reach, side="right") - 1
        widest = max(widest, int(np.max(last - np.arange(len(mem)))))
    return widest


def check_expected(label, E, bad, R):
    assert bad == 0 and np.isfinite(E).all(), bad
    err = np.abs(E.astype(np.float64) - R["expected"])
    with np.errstate(all="ignore"):      # (a diagonal pixel of one sub-fragment holds no pair: error 0 of tolerance 0)
        ratio = float(np.max(np.where(err > 0, err / R["tol"], 0.0)))
    print("%s: largest |E - E_ref| / tolerance %.3f" % (label, ratio))
    assert np.all(err <= R["tol"]), ratio
    assert np.array_equal(E, E.T) and np.all(E >= 0) and np.all(E[~np.eye(len(E), dtype=bool)] > 0)


def notices(R, d):
    """Pixels in which the brute force's part from cis pairs >= d slots apart exceeds the tolerance, against the count asked for."""
    n = R["far"][d]
    assert n >= 36 or R["m"] == 7, (d, n)                 # (49 pixels in all, see the module's docstring)
    return n


@pytest.mark.parametrize("name,max_px", STEPPED)
def test_shape_engages(name, max_px):
    P, s = problem(name)
    R = reference(name)[max_px]
    _, pxs, Sw, bins = CASES[name]
    n, lc = len(s["id_c"]), int(s["l_cont"].max())
    assert stripes_of(lc, n) == Sw and got(name, "stepped")["Sw"] == Sw and got(name, "fresh")["Sw"] == 1
    assert (-(-n // 64) * Sw + 3) // 4 > 1 and -(-n // 64) > 4             # k_mp_cis: blocks in the stepped state, tiles in any
    assert R["bin"] == bins[pxs.index(max_px)] and R["m"] == -(-int(P["init_n_sub_frags"]) // R["bin"])
    widest = window_slots(s, P["param_simu"][5])
    if name in ("m1", "m1_narrow"):
        assert lc >= 7745 and (s["circ"] == 1).any()                         # (the cap of 16 is what limits Sw)
        assert len(P["coo_row"]) > GRID_CONTACTS                            # k_mp_obs strides
    if name == "m1":
        assert widest > 64 * Sw + 64, widest                                 # every wave of a tile takes a second chunk
        notices(R, 64 * Sw)
    elif name == "m1_narrow":
        assert 64 < widest <= 128, widest                                    # lane + window < 3 chunks: waves 3 .. 15 of a tile leave at once
    else:
        assert widest > 64 and lc > 4 * widest and Sw >= 2, (widest, lc)
    if name == "m2":
        sid = np.asarray(P["np_sub_frags_id"]).reshape(-1, 4)
        assert (sid[:, 3] == 3).sum() > 2900 and (sid[:, 3] < 3).sum() >= 1 and (s["ori"] == -1).sum() >= 700
    if name == "m3":
        assert R["expected"].max() < 2.0 ** 29               # (bin 1: a pixel is one pair's term; one of 2^31 or more is a bad pixel by design)
        assert R["bin"] == 1 and (s["ori"] == -1).sum() >= 900 and (s["circ"] == 1).sum() == 400 and 2000 <= len(P["coo_row"]) <= 8000
    if max_px == 100:
        assert R["bin"] > 64                                                 # one run across all 64 lanes
    notices(R, FAR)


@pytest.mark.parametrize("name,max_px", STEPPED)
def test_order_and_observed(name, max_px):
    R = reference(name)[max_px]
    for engine_state in ("fresh", "stepped"):
        O, E, Rs, pix, b, bad = got(name, engine_state)[max_px]
        assert b == R["bin"] and O.shape == E.shape == Rs.shape == (R["m"], R["m"]), engine_state
        assert np.array_equal(pix, R["pixel_of_sub"]), engine_state
        assert O.dtype == np.float32 and np.array_equal(O, R["observed"]) and np.array_equal(O, O.T), engine_state
    assert O.sum(dtype=np.float64) > 0


@pytest.mark.parametrize("name,max_px", STEPPED)
def test_expected_equals_chunked_brute_force(name, max_px):
    """|E - E_ref| <= 1e-6 E_ref + terms 2^-30, tests/test_maps_gpu.py's bound (derived there), in both states."""
    R = reference(name)[max_px]
    for engine_state in ("fresh", "stepped"):
        G = got(name, engine_state)
        O, E, Rs, pix, b, bad = G[max_px]
        check_expected("%s max_px %d %s (Sw %d)" % (name, max_px, engine_state, G["Sw"]), E, bad, R)


@pytest.mark.parametrize("name", ["m1", "m1_narrow", "m2", "m3"])
def test_expected_conserves_the_full_evaluations_mass(name):
    """Half the sum of E (every pair once) is the expected mass the full evaluation subtracts: -eval_full_q()[1] / Q_SCALE."""
    for engine_state in ("fresh", "stepped"):
        G = got(name, engine_state)
        assert G["mass"] > 0
        for px in CASES[name][1]:
            half = float(G[px][1].sum(dtype=np.float64)) / 2.0
            print(name, engine_state, px, half, G["mass"])
            assert abs(half - G["mass"]) <= 1e-6 * G["mass"], (engine_state, px, half, G["mass"])


@pytest.mark.parametrize("name,max_px", STEPPED)
def test_residual(name, max_px):
    for engine_state in ("fresh", "stepped"):
        O, E, Rs, pix, b, bad = got(name, engine_state)[max_px]
        o, ex, r = (x.astype(np.float64) for x in (O, E, Rs))
        want = MR.residual(o, ex)
        # (tests/test_maps_gpu.py's bound: the device divides the float64 sums; O and E come back rounded to float32, so does R)
        tol = 2.0 ** -22 * ((np.abs(o) + np.abs(ex)) / np.sqrt(np.where(ex > 0, ex, 1.0)) + np.abs(want)) + 1e-30
        assert np.all(np.abs(r - want) <= tol), (engine_state, float(np.max(np.abs(r - want) / tol)))
        assert np.all(r[ex <= 0] == 0) and np.array_equal(Rs, Rs.T) and np.abs(r).max() > 0, engine_state


@pytest.mark.parametrize("name,max_px", STEPPED)
def test_fresh_and_stepped_agree_bit_for_bit(name, max_px):
    """The sums are int64 atomics: how many waves share a tile cannot show.  On m1 also a second stepped call at 4096 behind the calls
    at 100 and 7 (the buffers of 13 M pixels are reused)."""
    F, S = got(name, "fresh"), got(name, "stepped")
    for k in range(4):
        assert np.array_equal(F[max_px][k], S[max_px][k], equal_nan=True), k
    assert F[max_px][4:] == S[max_px][4:]
    if max_px == CASES[name][1][0] and "again" in S:
        for G in (F, S):
            for k in range(4):
                assert np.array_equal(G["again"][k], S[max_px][k], equal_nan=True), k
            assert G["again"][4:] == S[max_px][4:]
    print("%s: layout_maps at %s took %.2f s fresh, %.2f s stepped" % (name, CASES[name][1], F["seconds"], S["seconds"]))


def test_stale_stripes_equal_fresh():
    """m1_cut (211 contigs of at most 500 slots) behind a begin_step on m1's layout: 16 waves per tile where one would do, so almost
    every wave finds nothing behind its first chunk and leaves.  Bit for bit the fresh engine's images, and within the bound."""
    P, s = problem("m1_cut")
    R = reference("m1_cut")[100]
    F, S = got("m1_cut", "fresh"), got("m1_cut", "stale")
    assert (F["Sw"], S["Sw"]) == (1, 16) and stripes_of(s["l_cont"].max(), len(s["id_c"])) == 1 and int(s["l_cont"].max()) == 500
    assert R["bin"] == 110 and len(np.unique(s["id_c"])) > 200
    notices(R, FAR)
    for k in range(4):
        assert np.array_equal(F[100][k], S[100][k], equal_nan=True), k
    assert F[100][4:] == S[100][4:]
    O, E, Rs, pix, b, bad = S[100]
    assert b == R["bin"] and np.array_equal(pix, R["pixel_of_sub"]) and np.array_equal(O, R["observed"])
    check_expected("m1_cut max_px 100 stale (Sw 16)", E, bad, R)
