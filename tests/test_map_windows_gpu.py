"""graal_map_windows on the GPU: windows at bin 1 and at a layout map's own bin are crops of graal_layout_maps' images (pinned by
tests/test_maps_gpu.py), misaligned windows equal the numpy restatement (tests/window_map_reference.py), many windows in a call equal
each rendered alone, determinism and the independence of the two calls' buffers, no side effect on a run, the refusals, the junction
thumbnails and the CLI."""
import mmap
import os
import subprocess
import sys

import numpy as np
import pytest

from graal_amd import em, image, junctions, maps, synth
from graal_amd.lib import GraalError
from tests import map_reference as MR
from tests import window_map_reference as WMR
from tests.test_junctions_gpu import engine_for

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sub3", "sub1", "circ", "wide")
_full = {}


def full(name, max_px):
    """Engine.layout_maps of a case, computed once and shared (read only)."""
    if (name, max_px) not in _full:
        e = engine_for(MR.case(name))
        try:
            out = e.layout_maps(max_px)
        finally:
            e.close()
        for x in out[:4]:
            x.setflags(write=False)
        _full[(name, max_px)] = out
    return _full[(name, max_px)]


def crop(img, u0, v0, pr, pc, b):
    """The window at (u0, v0) (multiples of b) of the full image `img` of bin b, zero outside."""
    m = len(img)
    out = np.zeros((pr, pc), dtype=img.dtype)
    p0, q0 = u0 // b, v0 // b
    ps = [p for p in range(pr) if 0 <= p0 + p < m]
    qs = [q for q in range(pc) if 0 <= q0 + q < m]
    if ps and qs:
        out[ps[0]:ps[-1] + 1, qs[0]:qs[-1] + 1] = img[p0 + ps[0]:p0 + ps[-1] + 1, q0 + qs[0]:q0 + qs[-1] + 1]
    return out


def ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def check_crops(name, got, origins, pr, pc, max_px):
    """The rules of a window that is a crop of the full map at max_px: observed bit-identical, expected within one float32 ulp (both
    sides round the same real number, computed in float64 from the same integers), the residual within tests/test_maps_gpu.py's
    tolerance, pixels outside the genome exactly 0."""
    O, E, Rs, pix, b, bad = full(name, max_px)
    S = len(pix)
    obs, exp, res, rank, nbad = got
    assert obs.shape == exp.shape == res.shape == (len(origins), pr, pc) and obs.dtype == exp.dtype == res.dtype == np.float32
    assert nbad == 0 and bad == 0
    if b == 1:
        assert np.array_equal(rank, pix)
    else:
        assert np.array_equal(rank // b, pix)
    for w, (u0, v0) in enumerate(origins):
        assert u0 % b == 0 and v0 % b == 0
        assert np.array_equal(obs[w], crop(O, u0, v0, pr, pc, b)), (name, w)
        want = crop(E, u0, v0, pr, pc, b)
        assert np.all(np.abs(exp[w].astype(np.float64) - want) <= ulp32(want)), (name, w)
        o, ex, r = (x.astype(np.float64) for x in (obs[w], exp[w], res[w]))
        ref = MR.residual(o, ex)
        tol = 2.0 ** -22 * ((np.abs(o) + np.abs(ex)) / np.sqrt(np.where(ex > 0, ex, 1.0)) + np.abs(ref)) + 1e-30
        assert np.all(np.abs(r - ref) <= tol), (name, w)
        assert np.all(np.abs(r - crop(Rs, u0, v0, pr, pc, b)) <= tol), (name, w)
        rows = (u0 + b * np.arange(pr) >= S) | (u0 + b * (np.arange(pr) + 1) <= 0)
        cols = (v0 + b * np.arange(pc) >= S) | (v0 + b * (np.arange(pc) + 1) <= 0)
        outside = rows[:, None] | cols[None, :]
        for x in (obs[w], exp[w], res[w]):
            assert np.all(x[outside] == 0), (name, w)
    return sum(int((exp[w] != crop(E, u0, v0, pr, pc, b)).sum()) + int((res[w] != crop(Rs, u0, v0, pr, pc, b)).sum())
               for w, (u0, v0) in enumerate(origins))


def bin1_origins(name):
    """At least the seven windows of the bin-1 test, for a window of 30 x 30 or 30 x 41 pixels."""
    P = MR.case(name)
    S = int(P["init_n_sub_frags"])
    R = MR.reference(name, 4096)
    s = P["S_o_A_frags"]
    sid = np.asarray(P["np_sub_frags_id"]).reshape(-1, 4)
    label = np.zeros(S, dtype=np.int64)                       # per rank
    for f in range(len(sid)):
        label[R["pixel_of_sub"][sid[f, :sid[f, 3]]]] = s["id_c"][f]
    first = {int(c): int(np.nonzero(label == c)[0][0]) for c in np.unique(label)}
    labs = sorted(first)
    big = max(labs, key=lambda c: int((label == c).sum()))
    other = [c for c in labs if c != big][0]
    o = [[7, 7],                                              # on the diagonal at an odd origin
         [first[big], first[other]],                          # rows in one contig, columns in another
         [10, 25],                                            # rows [10, 40) against columns [25, 55) with 30 pixels: partial overlap
         [-5, -5], [-5, 3],                                   # origin -5
         [S - 11, S - 17],                                    # reaching past S
         [S + 3, 5], [-200, -100]]                            # wholly outside
    if name == "circ":
        ring = [int(c) for c in np.unique(s["id_c"][np.asarray(s["circ"]) == 1])]
        assert ring
        o.append([first[ring[0]] + 1, first[ring[0]] + 2])    # inside the ring
        o.append([first[ring[0]], first[ring[0]] + int((label == ring[0]).sum()) - 30])   # its two ends: across the wrap
    return np.array(o, dtype=np.int32)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("shape", [(30, 30), (30, 41)])
def test_bin_1_is_a_crop_of_the_full_map(name, shape):
    origins = bin1_origins(name)
    e = engine_for(MR.case(name))
    try:
        got = e.map_windows(origins, shape[0], shape[1], 1)
    finally:
        e.close()
    differ = check_crops(name, got, origins.tolist(), shape[0], shape[1], 4096)
    print("%s %s: %d expected / residual pixels differ from the crop in the last place" % (name, shape, differ))
    assert differ == 0      # the float64 operations are k_mp_out's (maps.h: mp_pixel): bit-identical, not only within an ulp
    assert got[0].sum() > 0 and got[1].max() > 0 and np.abs(got[2]).max() > 0


@pytest.mark.parametrize("name", NAMES)
def test_aligned_bins_are_crops_of_the_full_map(name):
    for max_px in MR.MAX_PX[name][1:]:
        b, m = MR.reference(name, max_px)["bin"], MR.reference(name, max_px)["m"]
        assert b > 1
        pr, pc = min(m, 6) + 1, min(m, 9) + 2
        origins = [[0, 0], [b * (m // 3), b * (m // 3)], [b * (m // 2), 0], [b * (m - 2), b * (m - 3)], [-b, 2 * b if m > 4 else 0],
                   [b * (m - 1), b * (m - 1)]]
        e = engine_for(MR.case(name))
        try:
            got = e.map_windows(origins, pr, pc, b)
        finally:
            e.close()
        differ = check_crops(name, got, origins, pr, pc, max_px)
        print("%s bin %d: %d expected / residual pixels differ from the crop in the last place" % (name, b, differ))
        assert differ == 0


def check_reference(got, W):
    """Observed exactly; |E - E_ref| <= 1e-6 E_ref + terms 2^-30 (tests/test_maps_gpu.py: test_expected_equals_brute_force derives it),
    `terms` the ordered pairs priced in the pixel."""
    obs, exp, res, rank, nbad = got
    assert nbad == 0 and np.array_equal(obs, W["observed"])
    err = np.abs(exp.astype(np.float64) - W["expected"])
    tol = 1e-6 * W["expected"] + W["terms"] * 2.0 ** -30
    with np.errstate(all="ignore"):
        ratio = float(np.max(np.where(err > 0, err / tol, 0.0)))
    print("largest |E - E_ref| / tolerance %.3f" % ratio)
    assert np.all(err <= tol), ratio
    o, ex, r = (x.astype(np.float64) for x in (obs, exp, res))
    ref = MR.residual(o, ex)
    rtol = 2.0 ** -22 * ((np.abs(o) + np.abs(ex)) / np.sqrt(np.where(ex > 0, ex, 1.0)) + np.abs(ref)) + 1e-30
    assert np.all(np.abs(r - ref) <= rtol)
    assert np.all(exp[W["terms"] == 0] == 0) and np.all(obs[W["terms"] == 0] == 0)


@pytest.mark.parametrize("name", NAMES)
def test_misaligned_bin_equals_the_reference(name):
    S = int(MR.case(name)["init_n_sub_frags"])
    origins = np.array([[3, 7], [7, 3], [3, 3], [S - 31, S - 44], [-12, 7]], dtype=np.int32)   # ([3, 3]: on the diagonal, pixels that
    W = WMR.windows(name, origins, 9, 13, 5)                                                    # share all their ranks; [3, 7]: part of them)
    e = engine_for(MR.case(name))
    try:
        got = e.map_windows(origins, 9, 13, 5)
        wide = e.map_windows([[3, 7], [7, 3]], 5, 3, 23)         # a wave per pixel (bin > 8), ragged at S
        huge = e.map_windows([[-100, -50], [0, 0]], 2, 2, 600)  # a block per pixel (bin > 512 ranks), its columns in two tiles
    finally:
        e.close()
    assert (W["terms"] == 25).any() and (W["terms"] == 20).any() and (W["terms"] == 25 - 1).any() and (W["terms"] == 0).any()
    check_reference(got, W)
    check_reference(wide, WMR.windows(name, [[3, 7], [7, 3]], 5, 3, 23))
    check_reference(huge, WMR.windows(name, [[-100, -50], [0, 0]], 2, 2, 600))
    assert np.array_equal(got[3], MR.reference(name, 4096)["pixel_of_sub"])


def test_many_windows_in_one_call():
    """1, 2 and 65 windows (more than a wave has lanes), duplicates and heavy overlaps: each image bit-identical to the same window
    rendered alone."""
    name = "wide"
    S = int(MR.case(name)["init_n_sub_frags"])
    rng = np.random.RandomState(9)
    many = np.concatenate([[[100, 100], [100, 100], [101, 100], [100, 101], [99, 99]], np.stack([100 + np.arange(40), 90 + 2 * np.arange(40)], 1),
                           rng.randint(-20, S + 10, size=(20, 2))]).astype(np.int32)
    assert len(many) == 65
    e = engine_for(MR.case(name))
    try:
        for b, pr, pc in ((1, 12, 17), (4, 6, 7), (11, 5, 4)):
            alone = {}
            for u0, v0 in {tuple(x) for x in many.tolist()}:
                alone[(u0, v0)] = e.map_windows([[u0, v0]], pr, pc, b)
            for n_win in (1, 2, 65):
                got = e.map_windows(many[:n_win], pr, pc, b)
                assert got[0].shape == (n_win, pr, pc)
                for w in range(n_win):
                    one = alone[tuple(many[w].tolist())]
                    for k in range(3):
                        assert np.array_equal(got[k][w], one[k][0], equal_nan=True), (b, n_win, w, k)
                assert np.array_equal(got[3], one[3])
            assert got[0].sum() > 0
    finally:
        e.close()


def test_deterministic_and_the_buffers_are_the_calls_own():
    e = engine_for(MR.case("wide"))
    try:
        A = ([[50, 60], [200, 190]], 20, 14, 3)
        B = ([[0, 0]], 64, 64, 1)
        a = e.map_windows(*A)
        b = e.map_windows(*B)
        full_map = e.layout_maps(50)                           # (the full maps' call in between changes neither side's fetch)
        obs, exp, res = (np.zeros((1, 64, 64), dtype=np.float32) for _ in range(3))
        rank = e.map_windows_fetch(obs, exp, res)
        for x, y in zip(b[:4], (obs, exp, res, rank)):
            assert np.array_equal(x, y, equal_nan=True)
        c = e.map_windows(*A)
        for k in range(4):
            assert np.array_equal(a[k], c[k], equal_nan=True), k
        assert a[4] == c[4] and b[0].shape == (1, 64, 64) and a[0].shape == (2, 20, 14)
        O, E, Rs = (np.zeros_like(full_map[0]) for _ in range(3))
        pix = e.layout_maps_fetch(O, E, Rs)
        for x, y in zip(full_map[:4], (O, E, Rs, pix)):
            assert np.array_equal(x, y, equal_nan=True)
        first = full("wide", 50)
        for k in range(4):
            assert np.array_equal(first[k], full_map[k], equal_nan=True), k
    finally:
        e.close()


def test_no_side_effect_on_a_run():
    """run_em with window_maps called behind every cycle gives the same accepted moves, likelihoods, contig counts and generator state."""
    from tests.test_sampler_gpu import make_gpu_sampler
    P = synth.with_dense(synth.make_problem(n_bins=70, nnz=1200, n_sub=1, seed=41, contig_weights=(5, 4, 3), mean_len_bp=2000.0,
                                            param=synth.make_param_simu(fact=200.0, v_inter=0.02), grid_bp=2000))
    runs = []
    for call in (False, True):
        rng = np.random.RandomState(5)
        smp = make_gpu_sampler(P, rng, reference_arithmetic="exact")
        seen = []

        def on_cycle(j, s, seen=seen):
            m = maps.window_maps(s, [[0, 0], [10, 30]], 70, 70, 1)
            seen.append((j, m["observed"].shape, float(m["observed"][0].astype(np.float64).sum())))

        tr = em.run_em(smp, 3, 3, rng=rng, on_cycle=on_cycle if call else None)
        runs.append((tr.mutations(), np.array(tr.likelihood), np.array(tr.n_contigs), rng.get_state()))
        smp.free_gpu()
        if call:
            assert [x[0] for x in seen] == [0, 1, 2] and all(x[1] == (2, 70, 70) for x in seen)
            assert all(x[2] == 2.0 * float(np.sum(P["coo_val"])) for x in seen)      # (70 x 70 at bin 1 from rank 0: the whole genome)
    (m0, l0, c0, g0), (m1, l1, c1, g1) = runs
    assert np.array_equal(m0, m1) and np.array_equal(c0, c1) and np.array_equal(l0, l1)
    assert g0[0] == g1[0] and np.array_equal(g0[1], g1[1]) and g0[2:] == g1[2:]


def test_refusals():
    e = engine_for(MR.case("sub1"))
    try:
        with pytest.raises(GraalError, match=r"code 3\)"):
            e.map_windows_fetch()
        for args in (([], 4, 4, 1), ([[0, 0]], 0, 4, 1), ([[0, 0]], 4, 0, 1), ([[0, 0]], 4097, 4, 1), ([[0, 0]], 4, 4097, 1), ([[0, 0]], 4, 4, 0),
                     ([[0, 0]], 4, 4, -3), (np.zeros((5, 2)), 4096, 1024, 1), (np.zeros((4097, 2)), 64, 64, 2)):
            with pytest.raises(GraalError, match=r"code 1\)"):
                e.map_windows(*args)
        with pytest.raises(GraalError, match=r"code 3\)"):     # (a refused call leaves nothing to fetch)
            e.map_windows_fetch()
        e.layout_maps(16)
        with pytest.raises(GraalError, match=r"code 3\)"):     # (nor does the full maps' call)
            e.map_windows_fetch()
        assert e.map_windows(np.zeros((4, 2)), 1, 1, 1)[0].shape == (4, 1, 1)
        assert e.map_windows([[0, 0]], 2, 2, 2 ** 31 - 1)[0][0, 0, 0] > 0      # one pixel holds the genome; the next lies beyond it
        seg = mmap.mmap(-1, max(e.exchange_bytes(2), mmap.PAGESIZE))   # (rank 0 of two: a world of one has no exchange)
        e.attach_exchange(seg, 0, 2, 0)
        with pytest.raises(GraalError, match="one rank"):
            e.map_windows([[0, 0]], 4, 4, 1)
        e.detach_exchange()
        assert e.map_windows([[0, 0]], 4, 4, 1)[0].shape == (1, 4, 4)
    finally:
        e.close()
    from tests.test_repeats_gpu import engine_with_repeats, rep_problem
    R = rep_problem(1, 7)
    e = engine_with_repeats(R, R["S_o_A_frags"])
    try:
        with pytest.raises(GraalError, match=r"code 4\)"):
            e.map_windows([[0, 0]], 8, 8, 1)
    finally:
        e.close()


def test_junction_thumbnails():
    """junction_windows (n 3, px 16, bin 1) plus one call: the crops of the bin-1 full map around each junction's rank."""
    name = "wide"
    P = MR.case(name)
    e = engine_for(P)
    try:
        soa = e.download_frags()
        score, _ = e.junction_scores()
        table = junctions.table_from(soa, score)
        rank = maps.rank_of_sub(soa, e.sub_id)
        origins, t = maps.junction_windows(table, soa, e.sub_id, rank, 3, 16, 1)
        m = maps.window_maps(e, origins, 16, bin=1)
    finally:
        e.close()
    O, E, Rs, pix, b, bad = full(name, 4096)
    assert b == 1 and np.array_equal(rank, pix) and np.array_equal(m["rank_of_sub"], pix) and len(origins) == 3
    assert np.all(np.diff(t["score"]) >= 0) and t["score"][0] == np.nanmin(table["score"])
    sid = np.asarray(e.sub_id).reshape(-1, 4)
    for w in range(3):
        g = int(t["right_frag"][w])
        centre = int(pix[sid[g, :sid[g, 3]]].min())                                      # the right fragment's first rank
        left = int(t["left_frag"][w])
        assert centre - 1 == int(pix[sid[left, :sid[left, 3]]].max())                    # (the join lies just before it)
        assert origins[w].tolist() == [centre - 8, centre - 8] and int(t["u0"][w]) == centre - 8
        for k, img in (("observed", O), ("expected", E), ("residual", Rs)):
            assert np.array_equal(m[k][w], crop(img, centre - 8, centre - 8, 16, 16, 1), equal_nan=True), (w, k)


def test_run_writes_junction_maps(tmp_path):
    """python -m graal_amd.run --maps-junctions 3 --maps-junction-px 16 writes nine images and a map_junctions.tsv of three rows, the
    scores ascending and each window's origin its right fragment's rank less 8."""
    P = synth.make_problem(n_bins=150, nnz=2000, n_sub=1, seed=14, contig_weights=(5, 3, 2))
    par = synth.make_param_simu(fact=300.0, v_inter=0.02)
    data, out = str(tmp_path / "data"), str(tmp_path / "out")
    synth.write_dataset(P, data)
    cmd = [sys.executable, "-m", "graal_amd.run", "--dataset", data, "--size-pyramid", "1", "--level", "0", "--cycles", "2",
           "--neighbours", "3", "--seed", "3", "--arithmetic", "exact", "--out", out, "--junctions", "--maps-junctions", "3",
           "--maps-junction-px", "16", "--no-fit", "--param", *[repr(float(x)) for x in par]]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    folder = os.path.join(out, "maps")
    assert sorted(os.listdir(folder)) == sorted(["junction_%03d_%s.tiff" % (i, k) for i in range(3) for k in ("observed", "expected", "residual")]
                                                + ["map_junctions.tsv"])
    lines = open(os.path.join(folder, "map_junctions.tsv")).read().splitlines()
    assert lines[0].split("\t") == list(maps.JUNCTION_MAP_COLUMNS) and len(lines) == 4
    rows = [l.split("\t") for l in lines[1:]]
    scores = [float(x[5]) for x in rows]
    assert scores == sorted(scores) and all(x[7] == "1" for x in rows)
    all_scores = [float(l.split("\t")[-1]) for l in open(os.path.join(out, "junctions.tsv")).read().splitlines()[1:]]
    assert scores == sorted(s for s in all_scores if np.isfinite(s))[:3]
    for i in range(3):
        imgs = [image.read_tiff_f32(os.path.join(folder, "junction_%03d_%s.tiff" % (i, k))) for k in ("observed", "expected", "residual")]
        assert all(x.shape == (16, 16) and x.dtype == np.float32 for x in imgs)
        assert np.array_equal(imgs[0], imgs[0].T) and (imgs[1][8, 8] == 0) and imgs[1][8, 7] > 0      # (centred on the diagonal)
