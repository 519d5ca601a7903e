"""Shared by tests/test_repeat_cases_cpu.py and tests/test_repeats_midsize_gpu.py: repeated bins (allow_repeats) at shapes where
k_rep_delta and k_rep_full run many blocks, a bin has three or four extra copies, K reaches 10 and the layout takes the late stage --
three problems, each on grid coordinates with one RF count ("exact": the default arithmetic against dense_for) and on generic
coordinates with mixed RF counts ("reference": set_mode(ref_trans_accu=True, strict=True) against ref_dense).

A case is a problem, ONE layout built on purpose (build_layout: conditions (a)-(g) below, which layout_kinds reads back from the layout
alone) and its proposals (proposals: five kinds of fA, each with K neighbours).  The oracle's answers are computed once per process
(oracle_results).  Nothing here opens the GPU: graal_amd.lib is imported by the callers, inside functions."""
import time

import numpy as np

from graal_amd import synth
from oracle import oracle as O

VARIANTS = ("exact", "reference")

# dup: the repeated bins; roles: the three that build_layout places by hand (two neighbours in id whose copies share the longest contig,
# then the LAST bin); n_extra: copies added to each; cuts: the contigs the ordinary fragments are dealt into, longest first (None: the
# random layout's own); seed: of the problem; lseed: of the layout and the proposals
PROBLEMS = {
    "many short contigs": dict(n_bins=320, n_sub=3, nnz=20000, dup=(7, 21, 150, 151, 319), roles=(150, 151, 319), n_extra=3, n_contigs=40, cuts=None, K=10,
                               seed=301, lseed=11),
    "late stage": dict(n_bins=700, n_sub=3, nnz=40000, dup=(3, 300, 301, 699), roles=(300, 301, 699), n_extra=3, n_contigs=8, cuts=(300, 200, 100, 60, 30, 10), K=5,
                       seed=302, lseed=12),
    "one sub-fragment per bin": dict(n_bins=600, n_sub=1, nnz=30000, dup=(5, 100, 101, 300, 450, 599), roles=(100, 101, 599), n_extra=4, n_contigs=60, cuts=None, K=10,
                                     seed=303, lseed=13),
}
CASES = [(name, v) for name in PROBLEMS for v in VARIANTS]

_cache = {}


def _cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def tolerance(variant, base):
    """On a candidate delta: 1e-7 |logL| on grid coordinates (tests/test_repeats_gpu.py), 2e-9 |logL| in reference arithmetic
    (tests/test_strict_windowed_gpu.py)."""
    return (1e-7 if variant == "exact" else 2e-9) * abs(base)


# ---- the problems
def _subs(P, b):
    ids = np.asarray(P["np_sub_frags_id"]).reshape(-1, 4)
    return [int(x) for x in ids[b, :ids[b, 3]]]


def plant_counts(P, dup, roles):
    """Counts of 10-14 (factorial_f's Stirling form under lik_double's middle branch) and of 15 and more (lik_double's own Stirling
    branch) in the repeated bins' rows: between two repeated bins, inside a repeated bin with several sub-fragments, and against
    ordinary bins.  Returns P with the sub-level and bin-level contact lists rewritten (still sorted by (row, column))."""
    S = int(P["init_n_sub_frags"])
    n = int(P["n_frags"])
    d0, d1, d2, d3 = [_subs(P, b) for b in list(roles) + [b for b in dup if b not in roles][:1]]
    ordinary = [_subs(P, b)[0] for b in (11, 40, 77, 123, 200, 250, 310) if b not in dup]
    plant = [(d0[0], d1[0], 12), (d2[0], ordinary[0], 10), (d2[0], ordinary[1], 14), (d0[-1], ordinary[2], 15), (d1[0], ordinary[3], 40),
             (d3[0], ordinary[4], 11), (d3[-1], ordinary[5], 23), (d1[-1], d3[0], 16), (d0[0], ordinary[6], 13)]
    if len(d0) > 1:
        plant.append((d0[0], d0[1], 17))
    if len(d1) > 2:
        plant.append((d1[0], d1[2], 10))
    key = P["coo_row"].astype(np.int64) * S + P["coo_col"]
    val = dict(zip(key.tolist(), P["coo_val"].tolist()))
    for a, b, c in plant:
        assert a != b
        val[min(a, b) * S + max(a, b)] = c
    keys = np.array(sorted(val), np.int64)
    p = dict(P)
    p["coo_row"], p["coo_col"] = (keys // S).astype(np.int32), (keys % S).astype(np.int32)
    p["coo_val"] = np.array([val[k] for k in keys.tolist()], np.int32)
    bos = np.asarray(P["bin_of_sub"])                      # the bin-level list, as synth.make_problem sums it
    bi, bj = bos[p["coo_row"]].astype(np.int64), bos[p["coo_col"]].astype(np.int64)
    m = bi != bj
    ub, inv = np.unique(np.minimum(bi[m], bj[m]) * n + np.maximum(bi[m], bj[m]), return_inverse=True)
    p["bin_coo_row"], p["bin_coo_col"] = (ub // n).astype(np.int32), (ub % n).astype(np.int32)
    p["bin_coo_val"] = np.bincount(inv, weights=p["coo_val"][m].astype(np.float64)).astype(np.float32)
    return p


def problem(name, variant):
    def make():
        c = PROBLEMS[name]
        if variant == "exact":
            from tests.test_repeats_gpu import rep_problem as base
        else:
            from tests.test_strict_windowed_gpu import rep_problem_ref as base
        P = base(c["n_sub"], c["seed"], n_bins=c["n_bins"], nnz=c["nnz"], dup=(), n_copies=0)      # (no repeats yet: the counts go in first)
        return synth.add_repeats(synth.with_dense(plant_counts(P, c["dup"], c["roles"])), c["dup"], c["n_extra"])
    return _cached(("problem", name, variant), make)


def dense(name, variant):
    def make():
        if variant == "exact":
            from tests.test_engine_gpu import dense_for as mk
        else:
            from tests.test_strict_windowed_gpu import ref_dense as mk
        return mk(problem(name, variant))
    return _cached(("dense", name, variant), make)


def engine(name, variant, state):
    """An engine with the case's problem and `state` uploaded, in the variant's arithmetic.  The caller closes it."""
    from tests.test_repeats_gpu import engine_with_repeats
    e = engine_with_repeats(problem(name, variant), state)
    if variant == "reference":
        e.set_mode(ref_trans_accu=True, strict=True)
    return e


# ---- the layout
def contigs_of(s):
    """The layout's contigs as lists of fragments in position order."""
    out = []
    for lab in np.unique(s["id_c"]):
        m = np.nonzero(s["id_c"] == lab)[0]
        out.append([int(f) for f in m[np.argsort(s["pos"][m], kind="stable")]])
    return out


def state_of(P, groups, circ, ori, inactive):
    """The layout whose contigs are `groups` (fragments in order; circ[i]: closed into a circle)."""
    S0 = P["S_o_A_frags"]
    n = int(P["n_new_frags"])
    s = O.new_state(n)
    for k in ("len_bp", "rep", "id_d"):
        s[k][:] = S0[k]
    s["id"][:] = np.arange(n)
    s["ori"][:] = ori
    s["activ"][:] = 1
    s["activ"][list(inactive)] = 0
    assert sorted(f for g in groups for f in g) == list(range(n))
    for lab, g in enumerate(groups):
        g = np.asarray(g, np.int64)
        lens = s["len_bp"][g].astype(np.int64)
        c = int(bool(circ[lab]) and len(g) >= 2)
        s["pos"][g] = np.arange(len(g))
        s["id_c"][g] = lab
        s["circ"][g] = c
        s["start_bp"][g] = np.cumsum(lens) - lens
        s["l_cont"][g] = len(g)
        s["l_cont_bp"][g] = lens.sum()
        s["prev"][g] = np.concatenate([[g[-1] if c else -1], g[:-1]])
        s["next"][g] = np.concatenate([g[1:], [g[0] if c else -1]])
    return s


def build_layout(P, seed, n_contigs, K, roles, cuts=None):
    """A random valid layout (random_state_with_repeats), its copies taken out and put back on purpose.  With roles = (d0, d1, d2)
    and the contigs by falling length L, M1, M2, C, G...:
      d0: two copies inside L (a, c), the third an inactive singleton (f: every other copy of d0 is active);
      d1: one copy inside L, next to none of d0's (b), one at position 0 of M1, one at the last position of M2 (d);
      d2: one copy, reversed, inside C, which is closed into a circle (e), one an inactive singleton (f);
      every other copy: active, at a random place of a contig that is not of kind (g).
    G: the next contigs of three fragments and more until they hold K + 2, freed of the repeated bins' originals (each changes places
    with an ordinary fragment of L) -- kind (g).  cuts: deal the ordinary fragments, in the random layout's order, into contigs of these
    lengths instead of the random layout's own (the late stage's long contigs are built, not met)."""
    from tests.test_repeats_gpu import random_state_with_repeats
    rng = np.random.RandomState(seed)
    s0 = random_state_with_repeats(P, rng, n_contigs=n_contigs, p_circ=0.25, p_inactive=0.0)
    rep = np.asarray(P["S_o_A_frags"]["rep"])
    id_d = np.asarray(P["S_o_A_frags"]["id_d"])
    dup = [int(b) for b in P["id_frag_duplicated"]]
    groups = [[f for f in g if rep[f] == 0] for g in contigs_of(s0)]
    groups = sorted([g for g in groups if g], key=len, reverse=True)
    if cuts is not None:
        flat = [f for g in groups for f in g]
        assert sum(cuts) == len(flat)
        ends = np.cumsum(cuts)
        groups = [flat[e - c:e] for c, e in zip(cuts, ends)]
    circ = [int(s0["circ"][g[0]]) for g in groups]
    ori = np.array(s0["ori"], copy=True)
    L, M1, M2, C = 0, 1, 2, 3
    assert len(groups) >= 5 and len(groups[C]) >= 3
    G, held = [], 0
    for i in range(4, len(groups)):
        if held < K + 2 and len(groups[i]) >= 3:
            G.append(i)
            held += len(groups[i])
    assert held >= K + 2, "not enough fragments in contigs of kind (g)"
    spare = [f for f in groups[L] if id_d[f] not in dup]
    for i in G:                                             # no original of a repeated bin in a contig of kind (g)
        for x, f in enumerate(groups[i]):
            if f in dup:
                o = spare.pop(int(rng.randint(len(spare))))
                groups[L][groups[L].index(o)] = f
                groups[i][x] = o
    circ[L], circ[M1], circ[M2], circ[C] = 0, 0, 0, 1
    copies = {b: [int(f) for f in np.nonzero((id_d == b) & (rep == 1))[0]] for b in dup}
    d0, d1, d2 = roles
    nL = len(groups[L])
    inactive = [copies[d0][2], copies[d2][1]]
    groups[L].insert(nL // 3, copies[d0][0])
    groups[L].insert(2 * nL // 3, copies[d0][1])
    groups[L].insert(nL // 2, copies[d1][0])
    groups[M1].insert(0, copies[d1][1])
    groups[M2].append(copies[d1][2])
    groups[C].insert(1, copies[d2][0])
    ori[copies[d2][0]] = -1
    ori[copies[d0][0]] = 1
    placed = set(inactive) | {copies[d0][0], copies[d0][1], copies[d1][0], copies[d1][1], copies[d1][2], copies[d2][0]}
    homes = [i for i in range(len(groups)) if i not in G]
    for b in dup:
        for f in copies[b]:
            if f not in placed:
                g = groups[homes[int(rng.randint(len(homes)))]]
                g.insert(int(rng.randint(len(g) + 1)), f)
    groups += [[f] for f in inactive]
    circ += [0] * len(inactive)
    return state_of(P, groups, circ, ori, inactive)


def layout(name, variant):
    """(layout, max_id) of a case, relabelled as the reference relabels (tests.test_engine_gpu.relabel_ref)."""
    def make():
        from tests.test_engine_gpu import relabel_ref
        c = PROBLEMS[name]
        s = build_layout(problem(name, variant), c["lseed"], c["n_contigs"], c["K"], c["roles"], c["cuts"])
        return s, relabel_ref(s)
    s, max_id = _cached(("layout", name, variant), make)
    return O.copy_state(s), max_id


def layout_kinds(P, s):
    """What a layout holds, read from the layout alone: conditions (a)-(g) as booleans, and the fragments that show them."""
    rep, activ, id_d = s["rep"], s["activ"], s["id_d"]
    dup = set(int(b) for b in P["id_frag_duplicated"])
    special = np.array([int(b) in dup for b in id_d])
    groups = contigs_of(s)
    longest = max(len(g) for g in groups)
    k = dict(a=False, b=False, c=False, d0=False, d1=False, e_circ=False, e_rev=False, g_contigs=[], inactive=[], lone_inactive=[],
             copies_in_long=[])
    for g in groups:
        cp = [f for f in g if rep[f] == 1]
        bins = [int(id_d[f]) for f in cp]
        k["a"] |= len(bins) != len(set(bins))
        k["b"] |= len(set(bins)) >= 2
        k["c"] |= len(g) == longest and len(cp) > 0
        k["d0"] |= len(g) >= 2 and rep[g[0]] == 1
        k["d1"] |= len(g) >= 2 and rep[g[-1]] == 1
        k["e_circ"] |= s["circ"][g[0]] == 1 and len(cp) > 0
        if len(g) >= 3 and not special[g].any():
            k["g_contigs"].append(g)
        if len(g) == longest:
            k["copies_in_long"] += [f for f in cp if 0 < s["pos"][f] < len(g) - 1 and activ[f] == 1]
    k["e_rev"] = bool(np.any((rep == 1) & (s["ori"] == -1) & (activ == 1)))
    for f in np.nonzero((rep == 1) & (activ == 0))[0]:
        assert s["l_cont"][f] == 1, "an inactive copy is a singleton contig"
        k["inactive"].append(int(f))
        others = np.nonzero((id_d == id_d[f]) & (np.arange(len(rep)) != f))[0]
        if np.all(activ[others] == 1):
            k["lone_inactive"].append(int(f))
    k["d"] = k["d0"] and k["d1"]
    k["e"] = k["e_circ"] and k["e_rev"]
    k["f"] = len(k["inactive"]) >= 2 and len(k["lone_inactive"]) >= 1
    k["g"] = len(k["g_contigs"]) >= 1
    return k


# ---- the proposals
PROPOSAL_KINDS = ("ordinary, beside a copy", "active copy in the longest contig", "inactive copy", "original of a repeated bin",
                  "away from every repeated bin")


def proposals(name, variant):
    """[(kind, fA, fBs)]: one proposal of every kind, each with K neighbours, none of them fA (the engine scores such a neighbour 0 on
    purpose).  Among the neighbours of the first four: a copy of fA's own bin (if it has copies), a copy of another repeated bin, an
    inactive copy, a fragment of fA's own contig (if it has company) and one of a contig of kind (g); the rest at random."""
    def make():
        c = PROBLEMS[name]
        P = problem(name, variant)
        s, _ = layout(name, variant)
        K = c["K"]
        rng = np.random.RandomState(c["lseed"] + 1000)
        kinds = layout_kinds(P, s)
        rep, id_d, id_c = s["rep"], s["id_d"], s["id_c"]
        n = len(rep)
        dup = [int(b) for b in P["id_frag_duplicated"]]
        g_frags = [f for g in kinds["g_contigs"] for f in g]
        beside = [f for f in range(n) if id_d[f] not in dup and s["pos"][f] > 0 and np.any((id_c == id_c[f]) & (rep == 1))
                  and s["l_cont"][f] < s["l_cont"].max()]
        fAs = [beside[int(rng.randint(len(beside)))], kinds["copies_in_long"][0], kinds["lone_inactive"][0], c["roles"][2]]
        out = []
        for kind, fA in zip(PROPOSAL_KINDS, fAs):
            own = [f for f in np.nonzero((id_d == id_d[fA]) & (rep == 1))[0] if f != fA]
            other = [f for f in np.nonzero((rep == 1) & (id_d != id_d[fA]) & (s["activ"] == 1))[0]]
            asleep = [f for f in kinds["inactive"] if f != fA]
            mates = [f for f in np.nonzero(id_c == id_c[fA])[0] if f != fA]
            fBs = []
            for pool in (own, other, asleep, mates, g_frags):
                pool = [int(f) for f in pool if int(f) not in fBs]
                if pool:
                    fBs.append(pool[int(rng.randint(len(pool)))])
            rest = np.setdiff1d(np.arange(n), fBs + [fA])
            fBs += [int(f) for f in rng.choice(rest, K - len(fBs), replace=False)]
            out.append((kind, int(fA), fBs))
        pick = [int(f) for f in rng.choice(g_frags, K + 1, replace=False)]
        out.append((PROPOSAL_KINDS[4], pick[0], pick[1:]))
        return out
    return _cached(("proposals", name, variant), make)


# ---- the oracle's answers, once per process
def oracle_results(name, variant):
    """dict(base, want=[K x 13 per proposal], seconds): DenseOracle.evaluate and oracle_deltas_with_repeats of every proposal."""
    def make():
        from tests.test_repeats_gpu import oracle_deltas_with_repeats
        P, D = problem(name, variant), dense(name, variant)
        s, max_id = layout(name, variant)
        t0 = time.time()
        base, want = None, []
        for _kind, fA, fBs in proposals(name, variant):
            base, w = oracle_deltas_with_repeats(P, D, s, fA, fBs, max_id)
            want.append(w)
        return dict(base=base, want=want, seconds=time.time() - t0)
    return _cached(("oracle", name, variant), make)


def plan_facts(name, variant):
    """What the step plan reads (step_plan.h: StepFacts), from the inputs alone -- as tests/step_plan_cases.run_case builds them."""
    from tests.test_repeats_gpu import split_observations
    c = PROBLEMS[name]
    P = problem(name, variant)
    s, max_id = layout(name, variant)
    row = split_observations(P)[0][0]
    n_sub = np.asarray(P["np_sub_frags_id"]).reshape(-1, 4)[:, 3]
    strict = int(variant == "reference")
    return dict(n=len(s["id_c"]), n_sub_total=int(P["init_n_sub_frags"]), nnz=len(row), single_sub=int(n_sub.max() == 1),
                n_contigs=max_id + 1, max_lcont=int(s["l_cont"].max()), lcont_bound=int(s["l_cont"].max()), has_rep=1, strict=strict,
                quirk=strict, K=c["K"], has_rowptr=int(np.all(np.diff(row) >= 0)), longest_row=int(np.bincount(row).max()),
                forced_producer=0)


# ---- the short run (problem 1, reference arithmetic)
RUN = dict(name="many short contigs", variant="reference", seed=7, delta=4,
           ids=(150, 320, 7, 151, 326, 21, 200, 323, 319, 60, 329, 332, 10, 321, 250, 327, 100, 333, 5, 330, 150, 324, 300, 334))


def oracle_run():
    """The oracle's side of the short run: dict(trace=[(id_fA, id_f_sampled, op)], likelihood=[...], stats=[...], final, seconds)."""
    def make():
        P = problem(RUN["name"], RUN["variant"])
        ora = O.OracleSampler(P, np.random.RandomState(RUN["seed"]), fix_trans_accu=False)
        t0 = time.time()
        ora.init_likelihood()
        trace, lik, stats = [], [], []
        for i in RUN["ids"]:
            r = ora.step_max_likelihood(int(i), RUN["delta"])
            trace.append((int(i), int(r[6]), int(r[5])))
            lik.append(float(r[0]))
            stats.append((int(r[1]), int(r[2]), int(r[4]), float(r[7])))
        return dict(trace=trace, likelihood=lik, stats=stats, final=O.copy_state(ora.gpu_vect_frags), seconds=time.time() - t0,
                    n_stale=ora.n_stale_paste)
    return _cached("run", make)
