"""graal_layout_maps on the GPU: order, binning and the observed image equal to the numpy restatement (tests/map_reference.py) and to
image.matrix_image, the expected image equal to the brute force over every sub-fragment pair and to the full evaluation's expected
mass, the residual, determinism, no side effect on a run, the meaning of the residual on simulated data, the refusals and the CLI."""
import os
import subprocess
import sys

import numpy as np
import pytest

from graal_amd import em, image, maps, synth
from graal_amd.lib import Engine, GraalError, Q_SCALE
from tests import map_reference as MR
from tests.test_junctions_gpu import _layout, engine_for

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(name, px) for name in ("sub3", "sub1", "circ", "wide") for px in MR.MAX_PX[name]]
_got = {}


def got(name, max_px):
    """Engine.layout_maps of a case, computed once and shared (read only)."""
    if (name, max_px) not in _got:
        e = engine_for(MR.case(name))
        try:
            out = e.layout_maps(max_px)
        finally:
            e.close()
        for x in out[:4]:
            x.setflags(write=False)
        _got[(name, max_px)] = out
    return _got[(name, max_px)]


@pytest.mark.parametrize("name,max_px", CASES)
def test_order_and_observed(name, max_px):
    P = MR.case(name)
    R = MR.reference(name, max_px)
    O, E, Rs, pix, b, bad = got(name, max_px)
    assert b == R["bin"] and O.shape == E.shape == Rs.shape == (R["m"], R["m"])
    assert np.array_equal(pix, R["pixel_of_sub"])
    assert O.dtype == np.float32 and np.array_equal(O, R["observed"]) and np.array_equal(O, O.T)
    if b == 1:
        assert np.array_equal(O, image.matrix_image((P["coo_row"], P["coo_col"], P["coo_val"]), R["order"], 4096))


@pytest.mark.parametrize("name,max_px", CASES)
def test_expected_equals_brute_force(name, max_px):
    """|E - E_ref| <= 1e-6 E_ref + terms 2^-30: the reference rounds a trans price three times in float32 (3 x 2^-24 relative), the device
    prices the background from exact integers in float64, a cis price may differ from numpy's by one float32 ulp: 4 x 2^-24 < 1e-6; and
    every pair's term is rounded to 2^-30 once."""
    R = MR.reference(name, max_px)
    O, E, Rs, pix, b, bad = got(name, max_px)
    err = np.abs(E.astype(np.float64) - R["expected"])
    tol = 1e-6 * R["expected"] + R["terms"] * 2.0 ** -30
    print("%s max_px %d: largest |E - E_ref| / tolerance %.3f, largest relative error %.3e" % (
        name, max_px, float(np.max(err / np.maximum(tol, 1e-300))), float(np.max(err / np.maximum(R["expected"], 1e-300)))))
    assert np.all(err <= tol), float(np.max(err / np.maximum(tol, 1e-300)))
    assert np.array_equal(E, E.T) and bad == 0 and np.all(E >= 0) and np.all(E[~np.eye(len(E), dtype=bool)] > 0)


@pytest.mark.parametrize("name", ["sub3", "sub1", "circ", "wide"])
def test_expected_conserves_the_full_evaluations_mass(name):
    """Half the sum of E (every pair once) is the expected mass the full evaluation subtracts: -eval_full_q()[1] / Q_SCALE."""
    e = engine_for(MR.case(name))
    try:
        sums = [float(e.layout_maps(px)[1].astype(np.float64).sum()) / 2.0 for px in MR.MAX_PX[name]]
        e.relabel_contigs()
        mass = -float(int(e.eval_full_q()[1])) / Q_SCALE
    finally:
        e.close()
    print(name, sums, mass)
    assert mass > 0
    for s in sums:
        assert abs(s - mass) <= 1e-6 * mass, (s, mass)


@pytest.mark.parametrize("name,max_px", CASES)
def test_residual(name, max_px):
    O, E, Rs, pix, b, bad = got(name, max_px)
    o, ex, r = (x.astype(np.float64) for x in (O, E, Rs))
    want = MR.residual(o, ex)
    # (the device divides the float64 sums; O and E come back rounded to float32, so does R)
    tol = 2.0 ** -22 * ((np.abs(o) + np.abs(ex)) / np.sqrt(np.where(ex > 0, ex, 1.0)) + np.abs(want)) + 1e-30
    assert np.all(np.abs(r - want) <= tol), float(np.max(np.abs(r - want) / tol))
    assert np.all(r[ex <= 0] == 0) and np.array_equal(Rs, Rs.T) and np.abs(r).max() > 0


def test_deterministic():
    first = got("wide", 50)
    e = engine_for(MR.case("wide"))
    try:
        a = e.layout_maps(50)
        b = e.layout_maps(7)      # (another shape in between: the buffers are reused)
        c = e.layout_maps(50)
    finally:
        e.close()
    assert b[0].shape == (7, 7)
    for x in (a, c):
        for k in range(4):
            assert np.array_equal(first[k], x[k], equal_nan=True), k
        assert x[4:] == first[4:]


def _sampler(P, rng):
    from tests.test_sampler_gpu import make_gpu_sampler
    return make_gpu_sampler(P, rng, reference_arithmetic="exact")


def test_no_side_effect_on_a_run():
    """run_em with layout_maps called behind every cycle gives the same accepted moves, likelihoods, contig counts and generator state."""
    P = synth.with_dense(synth.make_problem(n_bins=70, nnz=1200, n_sub=1, seed=41, contig_weights=(5, 4, 3), mean_len_bp=2000.0,
                                            param=synth.make_param_simu(fact=200.0, v_inter=0.02), grid_bp=2000))
    runs = []
    for call in (False, True):
        rng = np.random.RandomState(5)
        smp = _sampler(P, rng)
        seen = []

        def on_cycle(j, s, seen=seen):
            m = maps.layout_maps(s, 16)
            seen.append((j, m["observed"].shape, float(m["observed"].astype(np.float64).sum())))

        tr = em.run_em(smp, 3, 3, rng=rng, on_cycle=on_cycle if call else None)
        runs.append((tr.mutations(), np.array(tr.likelihood), np.array(tr.n_contigs), rng.get_state()))
        smp.free_gpu()
        if call:
            assert [x[0] for x in seen] == [0, 1, 2] and all(x[1] == (14, 14) for x in seen)
            assert all(x[2] == 2.0 * float(np.sum(P["coo_val"])) for x in seen)
    (m0, l0, c0, g0), (m1, l1, c1, g1) = runs
    assert np.array_equal(m0, m1) and np.array_equal(c0, c1) and np.array_equal(l0, l1)
    assert g0[0] == g1[0] and np.array_equal(g0[1], g1[1]) and g0[2:] == g1[2:]


def test_residual_of_simulated_data_is_standard_and_shows_an_inversion():
    """Contacts drawn from the model at the true layout: 2000 sub-fragments on 100 x 100 pixels of 20 x 20 pairs, every pixel's expected
    count >= 0.05 x 400 = 20, so a pixel is Poisson-like and its residual has mean 0 and variance 1.  The 9900 off-diagonal pixels are 4950
    independent ones: their mean has standard deviation 1 / sqrt(4950) = 0.014 and their variance sqrt(2 / 4950) = 0.02, far inside the
    bounds.  Then a block of 300 fragments (15 pixels; the window is about 6) of the first contig is inverted in the uploaded layout: the
    largest |residual| lies in a row or column of the block's pixels."""
    par = synth.make_param_simu(fact=2000.0, v_inter=0.05)
    P = synth.make_problem(n_bins=2000, nnz=500, n_sub=1, seed=13, contig_weights=(5, 3, 2), param=par)
    s = {k: np.asarray(v) for k, v in P["S_o_A_frags"].items()}
    e = Engine(0)
    try:
        e.upload_subfrags(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["init_n_sub_frags"],
                          P["mean_squared_frags_per_bin"])
        e.set_params(par)
        e.upload_frags(s)
        r, c, v = e.simulate_contacts(20260101)
        e.upload_contacts(r, c, v)
        O, E, R, pix, b, bad = e.layout_maps(100)
        assert (b, O.shape, bad) == (20, (100, 100), 0) and E.min() >= 19.99
        off = R[~np.eye(100, dtype=bool)].astype(np.float64)
        print("off-diagonal residuals: mean %.4f variance %.4f" % (off.mean(), off.var()))
        assert abs(off.mean()) <= 0.1
        assert 0.8 <= off.var() <= 1.25
        contigs = []
        for cid in np.unique(s["id_c"]):
            m = np.nonzero(s["id_c"] == cid)[0]
            contigs.append([(int(f), int(s["ori"][f])) for f in m[np.argsort(s["pos"][m])]])
        a = contigs[0]
        assert len(a) >= 900
        block = a[400:700]
        contigs[0] = a[:400] + [(f, -o) for f, o in block[::-1]] + a[700:]
        e.upload_frags(_layout(s["len_bp"], contigs))
        O2, E2, R2, pix2, b2, bad2 = e.layout_maps(100)
        rows = set(pix2[[f for f, _ in block]].tolist())      # (one sub-fragment per bin: its id is the fragment's)
        p, q = np.unravel_index(int(np.argmax(np.abs(R2))), R2.shape)
        assert np.abs(R2).max() > np.abs(R).max()
        assert int(p) in rows or int(q) in rows, (p, q, sorted(rows))
    finally:
        e.close()


def test_refusals():
    e = engine_for(MR.case("sub1"))
    try:
        with pytest.raises(GraalError, match=r"code 3\)"):
            e.layout_maps_fetch()
        for bad_px in (0, 4097):
            with pytest.raises(GraalError, match=r"code 1\)"):
                e.layout_maps(bad_px)
        with pytest.raises(GraalError, match=r"code 3\)"):     # (a refused call leaves nothing to fetch)
            e.layout_maps_fetch()
        assert e.layout_maps(1)[0].shape == (1, 1)
    finally:
        e.close()
    from tests.test_repeats_gpu import engine_with_repeats, rep_problem
    R = rep_problem(1, 7)
    e = engine_with_repeats(R, R["S_o_A_frags"])
    try:
        with pytest.raises(GraalError, match=r"code 4\)"):
            e.layout_maps(64)
    finally:
        e.close()


def test_run_writes_maps(tmp_path):
    """python -m graal_amd.run --maps --maps-every 1 --maps-max-px 64 writes the three images, the per-cycle ones and map_contigs.tsv; the
    images are Engine.layout_maps of the final layout (rebuilt here by replaying the run's list_mutations.txt; the contigs get the labels
    map_contigs.tsv lists for their head fragments)."""
    from graal_amd import pyramid as pyr
    from graal_amd.sampler import sampler
    P = synth.make_problem(n_bins=150, nnz=2000, n_sub=1, seed=14, contig_weights=(5, 3, 2))
    par = synth.make_param_simu(fact=300.0, v_inter=0.02)
    data, out = str(tmp_path / "data"), str(tmp_path / "out")
    synth.write_dataset(P, data)
    cmd = [sys.executable, "-m", "graal_amd.run", "--dataset", data, "--size-pyramid", "1", "--level", "0", "--cycles", "2",
           "--neighbours", "3", "--seed", "3", "--arithmetic", "exact", "--out", out, "--maps", "--maps-every", "1", "--maps-max-px", "64",
           "--no-fit", "--param", *[repr(float(x)) for x in par]]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    names = ("observed", "expected", "residual")
    final = {k: image.read_tiff_f32(os.path.join(out, k + ".tiff")) for k in names}
    for j in (0, 1):
        for k in names + ("map_contigs",):
            assert os.path.exists(os.path.join(out, "maps", "cycle_%05d_%s.%s" % (j, k, "tsv" if k == "map_contigs" else "tiff"))), (j, k)
    for k in names:      # (the last cycle's layout is the final one)
        assert np.array_equal(image.read_tiff_f32(os.path.join(out, "maps", "cycle_00001_%s.tiff" % k)), final[k], equal_nan=True)
    assert open(os.path.join(out, "maps", "cycle_00001_map_contigs.tsv")).read() == open(os.path.join(out, "map_contigs.tsv")).read()
    lines = open(os.path.join(out, "map_contigs.tsv")).read().splitlines()
    assert lines[0].split("\t") == list(maps.CONTIG_COLUMNS)
    rows = np.array([[int(x) for x in l.split("\t")] for l in lines[1:]], dtype=np.int64)
    n = int(rows[:, 1].sum())
    m = final["observed"].shape[0]
    assert m == -(-n // (-(-n // 64))) and np.all(np.diff(rows[:, 0]) > 0)
    assert rows[0, 2] == 0 and rows[-1, 3] == m - 1 and np.all(rows[1:, 2] >= rows[:-1, 3]) and np.all(rows[:, 2] <= rows[:, 3])
    # the final layout again: the same inputs, exploded, the run's accepted moves replayed
    inp = pyr.simulation_inputs(pyr.Pyramid(os.path.join(data, "pyramids", "pyramid_1_thresh_auto"), 1), 0)
    smp = sampler(True, inp["S_o_A_frags"], inp["collector_id_repeats"], inp["frag_dispatcher"], inp["id_frag_duplicated"],
                  inp["id_frags_blacklisted"], inp["n_frags"], inp["n_new_frags"], inp["init_n_sub_frags"], inp["n_new_sub_frags"],
                  None, inp["hic_matrix_sub_sampled"], inp["np_sub_frags_len_bp"], inp["np_sub_frags_id"], inp["np_sub_frags_accu"],
                  inp["mean_squared_frags_per_bin"], inp["norm_vect_accu"], inp["S_o_A_sub_frags"], inp["hic_matrix"],
                  inp["mean_value_trans"], 2, False, None, rng=np.random.RandomState(0), reference_arithmetic="exact")
    try:
        assert inp["n_frags"] == n
        smp.set_param_simu(np.asarray(par, dtype=np.float32))
        smp.modify_gl_cuda_buffer(0, 0)
        smp.explode_genome(0)
        em.replay(smp, em.load_mutations(os.path.join(out, "list_mutations.txt")))
        s = smp.engine.download_frags()
        assert len(np.unique(s["id_c"])) == len(rows) and np.array_equal(np.sort(np.nonzero(s["pos"] == 0)[0]), np.sort(rows[:, 4]))
        relabel = {int(s["id_c"][h]): int(lab) for lab, h in zip(rows[:, 0], rows[:, 4])}
        s["id_c"] = np.array([relabel[int(c)] for c in s["id_c"]], dtype=np.int32)
        smp.engine.upload_frags(s)
        got_maps = maps.layout_maps(smp, 64)
    finally:
        smp.free_gpu()
    for k in names:
        assert np.array_equal(got_maps[k], final[k], equal_nan=True), k
    for i, c in enumerate(maps.CONTIG_COLUMNS):
        assert np.array_equal(got_maps["contigs"][c], rows[:, i]), c
    assert final["observed"].sum() > 0 and np.array_equal(final["observed"], final["observed"].T)
