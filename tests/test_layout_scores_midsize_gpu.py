"""graal_junction_scores, graal_end_links / graal_end_links_best, graal_insertions and graal_edit_layout at mid-size shapes, against the
windowed restatement (tests/window_reference.py) and tests/edit_reference.py.  The shapes (tests/window_cases.py) reach what the small
problems never do: multi-stripe junction tiles up to the cap of 16 waves and a second tile per wave (on a STEPPED engine, one that ran
graal_begin_step behind the upload: the handle sizes k_jn_mass's and k_mp_cis's waves per tile by the longest contig of its last
begin_step, so a FRESH engine, upload only, runs one wave per tile whatever the layout, and a STALE one the waves of the layout before
-- tests/engine_states.py; the junction tests run in all three, the other tests' kernels do not read that statistic and run fresh), the window
exits, groups of 8 beyond the first on both sides of a link, grids that stride over more than 524,288 contacts, open-addressing tables
of thousands of keys, and 11 rounds of pointer jumping.  Keys and contact counts are compared for every link and insertion; Q and
status for every link and for a seeded sample of the insertions that covers each shape class.  Every test asserts that its shape
engages, and that each class of terms moves at least a few of the compared values by more than the tolerance (1e-9 * sum of |terms| +
1, in Q)."""
import numpy as np
import pytest

from graal_amd import links
from graal_amd.lib import JUNCTION_VALID, LINK_VALID, INSERT_VALID
from tests import edit_reference as ER
from tests import link_reference as LR
from tests import window_cases as WC
from tests import window_reference as WR
from tests.engine_states import GRID_CONTACTS, cached, engine_for, engine_in, stripes_of

pytestmark = pytest.mark.gpu
SAMPLE = 2048                           # insertions compared in full per table (the rest: keys and contacts only)


def problem(name):
    return cached(name, {"m1": WC.m1, "m2": WC.m2, "m1_cut": WC.m1_cut, "m2_cut": WC.m2_cut}[name])


def window(name, quirk):
    return cached((name, quirk), lambda: WR.window(problem(name), quirk))


def tol(A):
    return 1e-9 * np.asarray(A, np.float64) + 1


def _window_frags(s, reach):
    """Per end (2 * fragment + side) of every contig: how many of its fragments lie within reach bp of that end; -1 elsewhere."""
    n = len(s["id_c"])
    out = np.full(2 * n, -1, np.int64)
    for c, m in LR.contigs_of(s).items():
        off = np.cumsum(s["len_bp"][m]) - s["len_bp"][m]
        L = int(s["len_bp"][m].sum())
        out[2 * m[0]] = int((off <= reach).sum())
        out[2 * m[-1] + 1] = int((L - (off + s["len_bp"][m]) <= reach).sum())
    return out


def _sample(rng, m, classes):
    """A seeded sample of SAMPLE rows out of m, topped up with up to 24 rows of every class (a boolean mask over the rows)."""
    pick = set(rng.choice(m, min(m, SAMPLE), replace=False).tolist())
    for name, mask in classes.items():
        rows = np.nonzero(mask)[0]
        assert len(rows) >= 3, name
        pick.update(rng.choice(rows, min(len(rows), 24), replace=False).tolist())
    return np.array(sorted(pick))


def _classes_move(parts, A, names):
    for k in names:
        moved = sum(abs(p.get(k, 0)) > t for p, t in zip(parts, tol(A)))
        assert moved >= 3, (k, moved)


# ---- junctions -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,quirk", [("m1", False), ("m1", True), ("m2", False), ("m2", True)])
def test_junctions_equal_restatement(name, quirk):
    """On a fresh engine (one wave per x tile) and on a stepped one, where k_jn_mass runs the `stripes` waves per tile that the layout
    calls for; each against the restatement of the layout that engine holds, and the two against each other word for word (the sums are
    int64 atomics and a junction's score does not depend on its contig's label)."""
    P = problem(name)
    W = window(name, quirk)
    got = {}
    for engine_state in ("fresh", "stepped"):
        e, s, Sw = engine_in(engine_state, P, quirk=quirk)
        try:
            q, st = e.junction_scores_q()
        finally:
            e.close()
        got[engine_state] = (q, st)
        parts = {}
        J, rst, A = W.junction_scores(s, parts)
        linear = s["circ"] == 0
        lc = int(s["l_cont"][linear].max())
        stripes = min(16, -(-(-(-lc // 64)) // 8))          # k_jn_mass: waves per 64-slot tile of the longest contig
        assert Sw == (stripes if engine_state == "stepped" else 1), (engine_state, Sw, stripes)
        if name == "m1":
            widest = max(_window_frags(s, W.reach))
            assert lc > 8192 and stripes == 16 and widest > 1024, (lc, widest)      # the cap, and a second tile per wave
            assert len(P["coo_row"]) > GRID_CONTACTS and (s["circ"] == 1).any()
        else:
            assert lc > 1024 and stripes == 3, lc
            assert (s["l_cont_bp"][linear] > W.reach).all()                         # every contig leaves the window
        assert np.array_equal(st, rst)
        ok = st == JUNCTION_VALID
        assert ok.sum() >= linear.sum() - 10 and (q[~ok] == 0).all()
        excess = np.abs(q[ok] - J[ok]) / tol(A[ok])
        print("%s quirk %d %s: Sw %d, largest |q - J| / tolerance %.3e" % (name, quirk, engine_state, Sw, float(excess.max())))
        bad = np.nonzero(excess > 1)[0]
        assert len(bad) == 0, (engine_state, len(bad), np.nonzero(ok)[0][bad[:5]], (q[ok] - J[ok])[bad[:5]])
        classes = ("contacts", "near", "wide") + (("far",) if quirk and name == "m2" else ())
        for k in classes:
            assert (np.abs(parts[k][ok]) > tol(A[ok])).sum() >= 3, k
    assert np.array_equal(got["fresh"][0], got["stepped"][0]) and np.array_equal(got["fresh"][1], got["stepped"][1])
    if name == "m1" and not quirk:
        # the prefix-sum identity against direct sums, at 64-slot tile boundaries and the ends of the longest contig
        long_c = LR.contigs_of(s)[int(s["id_c"][np.argmax(np.where(linear, s["l_cont"], 0))])]
        at = [0, 1, 62, 63, 64, 127, 128, 1023, 1024, 1535, 4095, 4096, 8191, 8192, len(long_c) - 2]
        frags = [int(long_c[k]) for k in at]
        direct = W.junction_direct(s, frags)
        for f in frags:
            assert direct[f] == (J[f], False, A[f]), f


def test_junctions_with_stale_stripes():
    """m1_cut (longest contig 500: one wave per tile would do) uploaded behind a begin_step on m1's layout: k_jn_mass runs 16 waves per
    tile, of which almost every one finds nothing behind its first tile and leaves.  Equal to the fresh engine's scores word for word,
    and to the restatement."""
    P = problem("m1_cut")
    W = window("m1_cut", False)
    got = {}
    for engine_state in ("fresh", "stale"):
        e, s, Sw = engine_in(engine_state, P, before=problem("m1")["S_o_A_frags"])
        try:
            got[engine_state] = e.junction_scores_q()
        finally:
            e.close()
        assert Sw == (16 if engine_state == "stale" else 1)
        assert stripes_of(s["l_cont"].max(), len(s["id_c"])) == 1 and s["l_cont"].max() == 500
    q, st = got["stale"]
    assert np.array_equal(q, got["fresh"][0]) and np.array_equal(st, got["fresh"][1])
    parts = {}
    J, rst, A = W.junction_scores(s, parts)
    assert np.array_equal(st, rst)
    ok = st == JUNCTION_VALID
    assert ok.sum() >= 8000 and (q[~ok] == 0).all()
    excess = np.abs(q[ok] - J[ok]) / tol(A[ok])
    print("m1_cut stale: Sw 16, largest |q - J| / tolerance %.3e" % float(excess.max()))
    assert (excess <= 1).all(), int((excess > 1).sum())
    for k in ("contacts", "near", "wide"):
        assert (np.abs(parts[k][ok]) > tol(A[ok])).sum() >= 3, k


# ---- links ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,quirk,min_frags", [("m1_cut", False, 1), ("m1_cut", False, 3), ("m2_cut", False, 1), ("m2_cut", True, 1),
                                                  ("m2_cut", True, 5)])
def test_links_equal_restatement(name, quirk, min_frags):
    P = problem(name)
    s = P["S_o_A_frags"]
    W = window(name, quirk)
    e = engine_for(P, quirk=quirk)
    try:
        a, b, q, c, st = e.end_links_q(min_frags)
        be, bq, (ma, mb, mq) = e.end_links_best(min_frags)
    finally:
        e.close()
    ra, rb, rc = W.link_keys(s, min_frags)
    assert np.array_equal(a, ra) and np.array_equal(b, rb) and np.array_equal(c, rc)
    if name == "m1_cut":
        assert len(P["coo_row"]) > GRID_CONTACTS
        if min_frags == 1:
            assert len(a) >= 4096
    lc = s["l_cont"]
    wf = _window_frags(s, W.reach)
    fa, fb = a >> 1, b >> 1
    classes = {"groups_of_8": (wf[a] > 16) & (wf[b] > 16),                         # a second group of A and a second tile of B
               "exit": (s["l_cont_bp"][fa] > W.reach) | (s["l_cont_bp"][fb] > W.reach),
               "long": np.maximum(lc[fa], lc[fb]) > 256}
    if min_frags == 1:
        classes["single"] = np.minimum(lc[fa], lc[fb]) == 1
    for k, mask in classes.items():
        assert mask.sum() >= 3, k
    # every link's score and status
    parts = []
    rq, rst, A = W.link_scores(s, a, b, parts)
    assert np.array_equal(st, rst) and (rst == LINK_VALID).all()
    bad = np.nonzero(np.abs(q - rq) > tol(A))[0]
    assert len(bad) == 0, (len(bad), a[bad[:5]], b[bad[:5]], (q - rq)[bad[:5]])
    _classes_move(parts, A, ("contacts", "mass") + (("contacts_rest", "far", "mirror") if quirk else ()))
    moved = np.array([abs(p.get("mass", 0)) for p in parts]) > tol(A)
    assert (moved & classes["groups_of_8"]).sum() >= 3 and (moved & classes["exit"]).sum() >= 3
    if quirk:
        far = np.array([abs(p.get("far", 0)) for p in parts]) > tol(A)
        assert (far & classes["long"]).sum() >= 3
    # the best partners and the mutual-best links of the GPU's own table, ties included
    t = links.table_from(s, a, b, c, np.where(st == LINK_VALID, q.astype(np.float64), np.nan))      # (scores in Q: exact ties)
    best = links.best_links(t, 1)
    want_e = np.full(2 * len(s["id_c"]), -1, dtype=np.int64)
    want_q = np.zeros(2 * len(s["id_c"]), dtype=np.int64)
    ends = 2 * best["frag"] + best["side"]
    want_e[ends] = 2 * best["partner_frag"] + best["partner_side"]
    want_q[ends] = best["score"].astype(np.int64)
    assert len(ends) >= 20
    assert np.array_equal(be, want_e) and np.array_equal(bq, want_q)
    m = links.mutual_best(t)
    assert len(m["frag_a"]) >= 3
    assert np.array_equal(ma, 2 * m["frag_a"] + m["side_a"]) and np.array_equal(mb, 2 * m["frag_b"] + m["side_b"])
    assert np.array_equal(mq, m["score"].astype(np.int64))


# ---- insertions ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,quirk,max_frags", [("m1_cut", False, 1), ("m1_cut", False, 4), ("m2_cut", True, 1), ("m2_cut", True, 4),
                                                  ("m2_cut", False, 4)])
def test_insertions_equal_restatement(name, quirk, max_frags):
    P = problem(name)
    s = P["S_o_A_frags"]
    W = window(name, quirk)
    e = engine_for(P, quirk=quirk)
    try:
        p, f, r, q, c, st = e.insertions_q(max_frags)
        perm = np.random.RandomState(3).permutation(len(P["coo_row"]))
        e.upload_contacts(P["coo_row"][perm], P["coo_col"][perm], P["coo_val"][perm])
        shuffled = e.insertions_q(max_frags)
    finally:
        e.close()
    for x, y in zip((p, f, r, q, c, st), shuffled):
        assert np.array_equal(x, y)
    rp, rf, rr, rc = W.insertion_keys(s, max_frags)
    assert np.array_equal(p, rp) and np.array_equal(f, rf) and np.array_equal(r, rr) and np.array_equal(c, rc)
    if name == "m1_cut":
        assert len(P["coo_row"]) > GRID_CONTACTS
    lc = s["l_cont"]
    npf = lc[p]
    # junctions with several listed pieces of the same fragment count share their T1 x T2 term
    key = (f.astype(np.int64) * 8 + npf) * 2 + r
    _, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    classes = {"shared_t12": cnt[inv] >= 3, "exit": s["l_cont_bp"][f] > W.reach, "long": lc[f] > 256, "rev": r == 1}
    if max_frags > 1:
        classes["multi"] = npf == max_frags
    idx = _sample(np.random.RandomState(len(p)), len(p), classes)
    parts = []
    rq, rst, A = W.insertion_scores(s, p[idx], f[idx], r[idx], parts)
    assert np.array_equal(st[idx], rst) and (rst == INSERT_VALID).all()
    bad = np.nonzero(np.abs(q[idx] - rq) > tol(A))[0]
    assert len(bad) == 0, (len(bad), p[idx][bad[:5]], f[idx][bad[:5]], r[idx][bad[:5]], (q[idx] - rq)[bad[:5]])
    _classes_move(parts, A, ("contacts", "contacts_t12", "mass", "t12") + (("far", "mirror") if quirk else ()))
    t12 = np.array([abs(x.get("t12", 0)) for x in parts]) > tol(A)
    assert (t12 & classes["shared_t12"][idx]).sum() >= 3 and (t12 & classes["exit"][idx]).sum() >= 3


# ---- edit ----------------------------------------------------------------------------------------------------------------------------
def test_long_chain_edit_equals_restatement():
    """m1's 11,000 fragments cut 1,100 times (in every contig that spans several 256-fragment blocks, and the ring), then every piece
    chained into one contig by 1,105 joins in the same call: 11 rounds of pointer jumping."""
    P = problem("m1")
    s = P["S_o_A_frags"]
    n = len(s["id_c"])
    rng = np.random.RandomState(17)
    inner = np.nonzero((s["circ"] == 0) & (s["pos"] < s["l_cont"] - 1))[0]
    ring = np.nonzero(s["circ"] == 1)[0]
    cuts = [int(x) for x in rng.choice(inner, 1100, replace=False)] + [int(rng.choice(ring))]
    cut, _ = ER.edit(s, cuts, [])
    pieces = LR.contigs_of(cut)
    labs = [int(x) for x in rng.permutation(sorted(pieces))]
    joins, prev = [], None
    for c in labs:
        h, t = 2 * int(pieces[c][0]), 2 * int(pieces[c][-1]) + 1
        entry, exit_ = (h, t) if rng.rand() < 0.5 else (t, h)
        if prev is not None:
            joins.append((prev, entry) if rng.rand() < 0.5 else (entry, prev))
        prev = exit_
    rounds = 0
    while (1 << rounds) <= len(joins) + 1:
        rounds += 1
    assert n > 4096 and len(pieces) >= 1025 and len(joins) >= 1024 and rounds == 11
    big = [c for c, m in LR.contigs_of(s).items() if len(m) > 2 * 256]
    assert len(big) >= 2 and all(any(s["id_c"][f] == c for f in cuts) for c in big)
    want, st = ER.edit(s, cuts, joins)
    assert want is not None, st
    assert len(np.unique(want["id_c"])) == 1
    e = engine_for(P, s)
    try:
        got_st = e.edit_layout(cuts, joins)
        got = e.download_frags()
        assert not got_st.any()
        for k in LR.FIELDS:
            assert np.array_equal(got[k], want[k]), k
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
