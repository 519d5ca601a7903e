"""Scaffolding on the GPU: graal_end_links_best against the link table's best and mutual-best links, graal_edit_layout against the numpy
restatement (tests/edit_reference.py) and against an upload of the restated layout, and graal_amd.scaffold on simulated genomes cut into
shuffled pieces and with planted misjoins.  Small problems: the suite's GPU time stays small."""
import mmap
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from graal_amd import em, links, scaffold, synth
from graal_amd.lib import EDIT_CIRCULAR, EDIT_CYCLE, EDIT_END_TWICE, Engine, GraalError, LINK_VALID, Q_SCALE
from tests import edit_reference as ER
from tests import link_reference as LR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def engine_for(P, state=None, quirk=False):
    e = Engine(0)
    e.upload_subfrags(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["init_n_sub_frags"],
                      P["mean_squared_frags_per_bin"])
    e.upload_contacts(P["coo_row"], P["coo_col"], P["coo_val"])
    e.set_params(P["param_simu"])
    e.upload_frags(P["S_o_A_frags"] if state is None else state)
    if quirk:
        e.set_mode(ref_trans_accu=True)
    return e


_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = LR.case(name)
    return _CASES[name]


@pytest.mark.parametrize("name,quirk,min_frags", [("sub3", False, 1), ("sub3", True, 1), ("sub3", True, 3), ("sub1", False, 1),
                                                  ("sub1", True, 4), ("circ", False, 1)])
def test_best_partners_equal_the_link_table(name, quirk, min_frags):
    P = case(name)
    e = engine_for(P, quirk=quirk)
    try:
        a, b, q, c, st = e.end_links_q(min_frags)
        be, bq, (ma, mb, mq) = e.end_links_best(min_frags)
        a2, b2, q2, _, _ = e.end_links_q(min_frags)          # (the table call is unaffected)
    finally:
        e.close()
    assert np.array_equal(a, a2) and np.array_equal(b, b2) and np.array_equal(q, q2)
    s = P["S_o_A_frags"]
    t = links.table_from(s, a, b, c, np.where(st == LINK_VALID, q.astype(np.float64), np.nan))   # (scores in Q: exact ties)
    best = links.best_links(t, 1)
    want_e = np.full(2 * len(s["id_c"]), -1, dtype=np.int64)
    want_q = np.zeros(2 * len(s["id_c"]), dtype=np.int64)
    ends = 2 * best["frag"] + best["side"]
    want_e[ends] = 2 * best["partner_frag"] + best["partner_side"]
    want_q[ends] = best["score"].astype(np.int64)
    assert len(ends) > 0
    assert np.array_equal(be, want_e) and np.array_equal(bq, want_q)
    m = links.mutual_best(t)
    assert np.array_equal(ma, 2 * m["frag_a"] + m["side_a"]) and np.array_equal(mb, 2 * m["frag_b"] + m["side_b"])
    assert np.array_equal(mq, m["score"].astype(np.int64))


def random_layout(rng, lens, n_contigs, ring=True):
    n = len(lens)
    perm = rng.permutation(n)
    cuts = np.sort(rng.choice(np.arange(6, n), n_contigs - 1, replace=False))
    contigs = [[(int(f), int(rng.choice([-1, 1]))) for f in part] for part in np.split(perm, cuts)]
    return LR.layout(lens, contigs, {0} if ring else ())


def random_edit(rng, s, chain_len):
    """Random cuts (a ring cut included), then joins that chain random pieces of the cut layout, chain_len pieces per chain."""
    n = len(s["id_c"])
    inner = [f for f in range(n) if s["circ"][f] == 0 and s["pos"][f] < s["l_cont"][f] - 1]
    ring = [f for f in range(n) if s["circ"][f] == 1]
    cuts = [int(x) for x in rng.choice(inner, 3, replace=False)] + ([int(rng.choice(ring))] if ring else [])
    cut, _ = ER.edit(s, cuts, [])
    E = {c: (2 * int(m[0]), 2 * int(m[-1]) + 1) for c, m in LR.contigs_of(cut).items()}
    labs = [int(c) for c in rng.permutation(sorted(E))]
    joins = []
    for k in range(0, len(labs) - chain_len + 1, chain_len + 1):     # (a piece left out between chains)
        prev = None
        for c in labs[k:k + chain_len]:
            h, t = E[c]
            entry, exit_ = (h, t) if rng.rand() < 0.5 else (t, h)
            if prev is not None:
                joins.append((prev, entry) if rng.rand() < 0.5 else (entry, prev))
            prev = exit_
    return cuts, joins, E, labs


@pytest.mark.parametrize("name,seed,chain_len", [("sub3", 1, 2), ("sub3", 2, 3), ("sub1", 3, 4), ("sub1", 4, 3), ("sub3", 5, 5)])
def test_edit_equals_restatement(name, seed, chain_len):
    P = case(name)
    rng = np.random.RandomState(seed)
    s = random_layout(rng, P["S_o_A_frags"]["len_bp"], 9)
    cuts, joins, _, _ = random_edit(rng, s, chain_len)
    want, st = ER.edit(s, cuts, joins)
    assert want is not None, st
    e = engine_for(P, s)
    try:
        got_st = e.edit_layout(cuts, joins)
        got = e.download_frags()
        assert not got_st.any()
        for k in LR.FIELDS:
            assert np.array_equal(got[k], want[k]), k
        # after a relabel, the same as an upload of the restated layout
        e.relabel_contigs()
        q1 = e.eval_full_q()
        relabelled = e.download_frags()
        e.upload_frags(want)
        e.relabel_contigs()
        q2 = e.eval_full_q()
        assert np.array_equal(q1, q2)
        assert np.array_equal(relabelled["id_c"], e.download_frags()["id_c"])
    finally:
        e.close()


def test_edit_refusals_leave_the_layout():
    P = case("sub3")
    rng = np.random.RandomState(8)
    s = random_layout(rng, P["S_o_A_frags"]["len_bp"], 6)
    E = {c: (2 * int(m[0]), 2 * int(m[-1]) + 1) for c, m in LR.contigs_of(s).items()}
    e = engine_for(P, s)
    try:
        before = e.download_frags()
        cases = [([(E[1][1], E[2][0]), (E[2][1], E[3][0]), (E[3][1], E[1][0])], [EDIT_CYCLE] * 3),
                 ([(E[1][1], E[2][0]), (E[1][1], E[3][0])], [EDIT_END_TWICE] * 2),
                 ([(E[0][0], E[2][0])], [EDIT_CIRCULAR])]
        for joins, want in cases:
            with pytest.raises(GraalError, match=r"code 1\)") as ex:
                e.edit_layout([], joins)
            assert ex.value.status.tolist() == want
            assert ER.edit(s, [], joins)[1].tolist() == want
            after = e.download_frags()
            for k in LR.FIELDS:
                assert np.array_equal(after[k], before[k]), k
        seg = mmap.mmap(-1, max(e.exchange_bytes(2), mmap.PAGESIZE))
        e.attach_exchange(seg, 0, 2, 0)
        with pytest.raises(GraalError, match="one rank"):
            e.edit_layout([], [(E[1][1], E[2][0])])
        with pytest.raises(GraalError, match="one rank"):
            e.end_links_best(1)
        e.detach_exchange()
    finally:
        e.close()
    from tests.test_repeats_gpu import engine_with_repeats, rep_problem
    R = rep_problem(1, 7)
    e = engine_with_repeats(R, R["S_o_A_frags"])
    try:
        with pytest.raises(GraalError, match=r"code 4\)"):
            e.edit_layout([], [(0, 3)])
        with pytest.raises(GraalError, match=r"code 4\)"):
            e.end_links_best(1)
    finally:
        e.close()


def test_run_after_edit_equals_run_after_upload():
    """A seeded run_em after edit_layout gives the moves and likelihoods of one after upload_frags of the restated layout."""
    from tests.test_sampler_gpu import make_gpu_sampler
    P = synth.with_dense(synth.make_problem(n_bins=70, nnz=1200, n_sub=1, seed=41, contig_weights=(5, 4, 3), mean_len_bp=2000.0,
                                            param=synth.make_param_simu(fact=200.0, v_inter=0.02), grid_bp=2000))
    s = {k: np.asarray(v) for k, v in P["S_o_A_frags"].items()}
    lists = LR.contig_lists(s)
    labs = sorted(lists)
    cuts = [int(lists[labs[0]][10][0])]
    cut, _ = ER.edit(s, cuts, [])
    E = {c: (2 * int(m[0]), 2 * int(m[-1]) + 1) for c, m in LR.contigs_of(cut).items()}
    ks = sorted(E)
    joins = [(E[ks[0]][0], E[ks[1]][0]), (E[ks[1]][1], E[ks[3]][1])]
    want, st = ER.edit(s, cuts, joins)
    assert want is not None, st
    runs = []
    for via_edit in (True, False):
        rng = np.random.RandomState(5)
        smp = make_gpu_sampler(P, rng, reference_arithmetic="exact")
        if via_edit:
            smp.edit_layout(cuts, joins)
        else:
            smp.engine.upload_frags(want)
            smp.likelihood_t = None
        tr = em.run_em(smp, 2, 3, rng=rng, scrambled=False)
        runs.append((tr.mutations(), np.array(tr.likelihood), np.array(tr.n_contigs)))
        smp.free_gpu()
    (m0, l0, c0), (m1, l1, c1) = runs
    assert np.array_equal(m0, m1) and np.array_equal(c0, c1) and np.array_equal(l0, l1)


def simulated(seed_contacts=2024, par=None, weights=(4, 3, 2, 1)):
    par = synth.make_param_simu(fact=1500.0, v_inter=0.5) if par is None else par
    P = synth.make_problem(n_bins=1000, nnz=500, n_sub=1, seed=11, contig_weights=weights, param=par)
    s = {k: np.asarray(v) for k, v in P["S_o_A_frags"].items()}
    e = Engine(0)
    e.upload_subfrags(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["init_n_sub_frags"],
                      P["mean_squared_frags_per_bin"])
    e.set_params(par)
    e.upload_frags(s)
    r, c, v = e.simulate_contacts(seed_contacts)
    e.upload_contacts(r, c, v)
    return e, s


def assert_true_chromosomes(got, s):
    truth = LR.contigs_of(s)
    assert len(np.unique(got["id_c"])) == len(truth)
    for c, m in truth.items():
        lab = np.unique(got["id_c"][m])
        assert len(lab) == 1
        order = list(m[np.argsort(got["pos"][m])])
        assert order == list(m) or order == list(m[::-1])


@pytest.mark.parametrize("seed", [2024, 7, 99])
def test_scaffolding_recovers_the_chromosomes(seed):
    """The links test's genome: 4 chromosomes cut into 80-bin pieces, shuffled, about half reversed; scaffold rebuilds every chromosome."""
    e, s = simulated()
    try:
        rng = np.random.RandomState(seed)
        pieces = []
        for c, frags in LR.contig_lists(s).items():
            pieces += [frags[i:i + 80] for i in range(0, len(frags), 80)]
        flip = rng.rand(len(pieces)) < 0.5
        shuffled = [[(f, -o) for f, o in reversed(pieces[p])] if flip[p] else pieces[p] for p in rng.permutation(len(pieces))]
        e.upload_frags(LR.layout(s["len_bp"], shuffled))
        rec = scaffold.scaffold(e, rounds=20)
        got = e.download_frags()
    finally:
        e.close()
    kept = [r["logL"] for r in rec if r["kept"]]
    assert all(b >= a for a, b in zip(kept, kept[1:])), rec
    assert sum(r["joins"] for r in rec if r["kept"]) == len(pieces) - 4, rec
    assert_true_chromosomes(got, s)


def test_polishing_cuts_planted_misjoins():
    par = synth.make_param_simu(fact=300.0, v_inter=0.02)
    e, s = simulated(par=par, weights=(5, 3, 2))
    try:
        contigs = [list(v) for v in LR.contig_lists(s).values()]
        a, b = contigs[0], contigs[1]
        ha, hb = len(a) // 2, len(b) // 2
        contigs[0], contigs[1] = a[:ha] + b[hb:], b[:hb] + a[ha:]
        e.upload_frags(LR.layout(s["len_bp"], contigs))
        rec = scaffold.scaffold(e, rounds=10, cut_below=0.0)
        got = e.download_frags()
    finally:
        e.close()
    assert rec[1]["cuts"] == 2 and rec[1]["kept"] == 1, rec
    assert_true_chromosomes(got, s)


def test_run_scaffold_and_polish_write_their_tables():
    P = synth.make_problem(n_bins=300, nnz=3000, n_sub=1, seed=12, contig_weights=(5, 3, 2))
    with tempfile.TemporaryDirectory() as d:
        data, out = os.path.join(d, "data"), os.path.join(d, "out")
        synth.write_dataset(P, data)
        cmd = [sys.executable, "-m", "graal_amd.run", "--dataset", data, "--size-pyramid", "1", "--level", "0", "--cycles", "1",
               "--neighbours", "3", "--seed", "3", "--arithmetic", "exact", "--out", out, "--scaffold", "--polish",
               "--no-fit", "--param", *[str(float(x)) for x in synth.make_param_simu(fact=300.0, v_inter=0.02)]]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        for name in ("scaffold.tsv", "polish.tsv"):
            lines = open(os.path.join(out, name)).read().splitlines()
            assert lines[0].split("\t") == list(scaffold.COLUMNS)
            rows = [l.split("\t") for l in lines[1:]]
            assert rows[0][0] == "0" and len(rows) >= 1
        rows = [l.split("\t") for l in open(os.path.join(out, "scaffold.tsv")).read().splitlines()[1:]]
        assert len(rows) >= 2 and int(rows[1][2]) > 0        # (the exploded layout: the first round joins)
