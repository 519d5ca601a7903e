"""The case list of the tests that hold the oracle, the host build of frag_ops.h and the engine to the REFERENCE'S OWN
kernels (oracle/ref_kernels.py live on the CPU, tests/golden/ref_*.npz recorded for the GPU): seeded, deterministic, small.

A *layout* is a synthetic problem plus a random valid fragment layout, relabelled so that contig labels are ranks.  A
*proposal* is a fragment fA with K = 3 neighbours fB, as one step of the sampler evaluates them; its three (fA, fB) pairs
are the mutation cases.  The proposals are chosen greedily so that every class of pair in CLASSES -- the places where a
restatement of the mutation and likelihood kernels goes wrong -- occurs at least MIN_PER_CLASS times; that is asserted
when this module is imported, on the CPU and again by the GPU tests.
"""
import hashlib

import numpy as np

from graal_amd import synth
from oracle import oracle as O
from tests.test_engine_gpu import random_state_for, relabel_ref
from tests.test_repeats_gpu import random_state_with_repeats

K = 3
MIN_PER_CLASS = 8
MIN_PROPOSALS_PER_LAYOUT = 3   # every layout is exercised, also once the classes are full
MAX_PROPOSALS_PER_LAYOUT = 5
SENTINEL = -7   # prefill of a candidate's output slot (tests/test_oracle_golden.py::test_stale_paste_slot uses the same)

# name, n_sub, RF counts, bins, seed, p_circ, grid lengths?, repeated bins, contigs
LAYOUT_SPECS = [
    ("lin_1sub_grid", 1, 1, 24, 301, 0.0, True, (), 7),
    ("lin_3sub_mixed_generic", 3, ("random", 1, 9), 32, 302, 0.0, False, (), 9),
    ("circ_1sub_generic", 1, 1, 30, 303, 0.4, False, (), 8),
    ("circ_3sub_uniform_grid", 3, 9, 36, 304, 0.4, True, (), 9),
    ("circ_3sub_mixed_generic", 3, ("random", 1, 9), 40, 305, 0.4, False, (), 10),
    ("rep_1sub_grid", 1, 1, 26, 306, 0.0, True, (4, 15, 20), 12),
    ("rep_3sub_uniform_grid", 3, 9, 30, 307, 0.3, True, (5, 18, 22), 13),
]

POSITIONS = ("head", "tail", "middle", "singleton")
CLASSES = (tuple("A_" + p for p in POSITIONS) + tuple("B_" + p for p in POSITIONS) +
           ("same_contig_adjacent", "same_contig_not_adjacent", "different_contigs",
            "A_circular", "B_circular", "both_in_one_circular", "A_or_B_reversed",
            "A_is_B", "A_or_B_inactive", "A_copy_of_repeated_bin"))


def _problem(n_sub, accu, n_bins, seed, grid, dup):
    par = synth.make_param_simu(fact=300.0, v_inter=0.03)
    P = synth.make_problem(n_bins=n_bins, nnz=25 * n_bins, n_sub=n_sub, seed=seed, contig_weights=(5, 3, 2),
                           mean_len_bp=1500.0, accu=accu, param=par, grid_bp=2000 if grid else None)
    P = synth.with_dense(P)
    if len(dup):
        P = synth.add_repeats(P, dup, 2)
    return P


def _position(s, f):
    if s["l_cont"][f] == 1:
        return "singleton"
    if s["pos"][f] == 0:
        return "head"
    if s["pos"][f] == s["l_cont"][f] - 1:
        return "tail"
    return "middle"


def classes_of(s, fA, fB):
    """The classes of CLASSES the pair (fA, fB) of layout s belongs to."""
    out = {"A_" + _position(s, fA), "B_" + _position(s, fB)}
    same = s["id_c"][fA] == s["id_c"][fB]
    if fA == fB:
        out.add("A_is_B")
    elif same:
        out.add("same_contig_adjacent" if abs(int(s["pos"][fA]) - int(s["pos"][fB])) == 1 else "same_contig_not_adjacent")
    else:
        out.add("different_contigs")
    if s["circ"][fA] == 1:
        out.add("A_circular")
    if s["circ"][fB] == 1:
        out.add("B_circular")
    if same and fA != fB and s["circ"][fA] == 1:
        out.add("both_in_one_circular")
    if s["ori"][fA] == -1 or s["ori"][fB] == -1:
        out.add("A_or_B_reversed")
    if s["activ"][fA] == 0 or s["activ"][fB] == 0:
        out.add("A_or_B_inactive")
    if s["rep"][fA] == 1:
        out.add("A_copy_of_repeated_bin")
    return out


def _digest(P, s):
    """First 8 bytes of a SHA-256 over everything a kernel reads: a drift of synth or random_layout changes it."""
    h = hashlib.sha256()
    for k in O.FIELDS:
        h.update(np.ascontiguousarray(s[k], dtype=np.int32).tobytes())
    for k, dt in (("np_sub_frags_id", np.int32), ("np_sub_frags_len_bp", np.float32), ("np_sub_frags_accu", np.int32),
                  ("frag_dispatcher", np.int32), ("collector_id_repeats", np.int32), ("hic_matrix", np.float32),
                  ("param_simu", np.float32)):
        h.update(np.ascontiguousarray(P[k], dtype=dt).tobytes())
    h.update(np.float32(P["mean_squared_frags_per_bin"]).tobytes())
    return int.from_bytes(h.digest()[:8], "little") >> 1   # fits an int64


def _choose_proposals(s, rng, counts):
    """Greedy: the proposal (fA, three fB) that adds most to the classes still short of MIN_PER_CLASS, until none adds."""
    n = len(s["pos"])
    proposals = []
    order_a = [int(v) for v in rng.permutation(n)]
    order_b = [int(v) for v in rng.permutation(n)]
    while len(proposals) < MAX_PROPOSALS_PER_LAYOUT:
        best = None
        for fA in order_a:
            if any(fA == p[0] for p in proposals):
                continue
            local = dict(counts)
            fBs, gain = [], 0
            for _ in range(K):
                pick, pick_gain = None, -1
                for fB in order_b:
                    if fB in fBs:
                        continue
                    g = sum(1 for c in classes_of(s, fA, fB) if local[c] < MIN_PER_CLASS)
                    if g > pick_gain:
                        pick, pick_gain = fB, g
                fBs.append(pick)
                gain += pick_gain
                for c in classes_of(s, fA, pick):
                    local[c] += 1
            if best is None or gain > best[0]:
                best = (gain, fA, fBs)
        if best is None or (best[0] == 0 and len(proposals) >= MIN_PROPOSALS_PER_LAYOUT):
            break
        proposals.append((best[1], best[2]))
        for fB in best[2]:
            for c in classes_of(s, best[1], fB):
                counts[c] += 1
    return proposals


def _build():
    layouts, counts = [], {c: 0 for c in CLASSES}
    for name, n_sub, accu, n_bins, seed, p_circ, grid, dup, n_contigs in LAYOUT_SPECS:
        P = _problem(n_sub, accu, n_bins, seed, grid, dup)
        rng = np.random.RandomState(seed)
        if len(dup):
            s = random_state_with_repeats(P, rng, n_contigs=n_contigs, p_circ=p_circ, p_inactive=0.7)
            # two more copies inactive, the way a run gets them: op 8 (eject, then swap the activity) on an active copy
            from tests import util
            for f in [int(v) for v in np.nonzero((s["rep"] == 1) & (s["activ"] == 1))[0][:2]]:
                s, _ = util.oracle_candidate(s, f, f, 8, relabel_ref(s))
            util.check_invariants(s)
        else:
            s = random_state_for(P, rng, n_contigs=n_contigs, p_circ=p_circ)
        max_id = relabel_ref(s)
        lay = {"name": name, "P": P, "state": s, "max_id": int(max_id), "repeats": bool(len(dup)), "n_sub": n_sub,
               "mixed_rf": isinstance(accu, tuple), "digest": _digest(P, s)}
        lay["proposals"] = _choose_proposals(s, rng, counts)
        layouts.append(lay)
    return layouts, counts


LAYOUTS, CLASS_COUNTS = _build()
PAIRS = [(li, fA, fB) for li, lay in enumerate(LAYOUTS) for fA, fBs in lay["proposals"] for fB in fBs]

# -- the coverage this list exists for -----------------------------------------------------------------------------------
assert all(24 <= len(lay["state"]["pos"]) <= 40 for lay in LAYOUTS)
assert all(CLASS_COUNTS[c] >= MIN_PER_CLASS for c in CLASSES), {c: v for c, v in CLASS_COUNTS.items() if v < MIN_PER_CLASS}
assert sum(1 for lay in LAYOUTS if not lay["repeats"] and not (lay["state"]["circ"] == 1).any()) >= 2
assert sum(1 for lay in LAYOUTS if (lay["state"]["circ"] == 1).any()) >= 2
assert sum(1 for lay in LAYOUTS if lay["repeats"] and (lay["state"]["activ"] == 0).any()) >= 2
assert {lay["n_sub"] for lay in LAYOUTS} == {1, 3} and any(lay["mixed_rf"] for lay in LAYOUTS)


def kernels_for(lay, cls):
    """The layout's data behind a kernel class (oracle.DenseOracle or ref_kernels.RefKernels), reference indexing."""
    P = lay["P"]
    return cls(P["hic_matrix"], P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"],
               P["frag_dispatcher"], P["collector_id_repeats"], P["n_frags"], P["mean_squared_frags_per_bin"],
               P["param_simu"], fix_trans_accu=False)


def pixel_lists(lay, state, fA, fB):
    """(no_rep, reps, uniq): the lists stream_likelihood hands to sub_compute_likelihood (cuda_lib_gl.py:2453-2458; as
    tests/test_repeats_gpu.oracle_deltas_with_repeats builds them)."""
    P = lay["P"]
    dup = np.asarray(P.get("id_frag_duplicated", []), dtype=np.int32)
    uniq = np.setdiff1d(np.arange(P["n_frags"], dtype=np.int32), dup)
    in_ab = np.nonzero((state["id_c"] == state["id_c"][fA]) | (state["id_c"] == state["id_c"][fB]))[0]
    sub_index = state["id_d"][in_ab]
    return np.setdiff1d(sub_index, dup), np.intersect1d(sub_index, dup), uniq


def restricted_pixels(n_bins, no_rep, reps, uniq):
    """Indices into the per-pixel vector of the pixels sub_compute_likelihood visits, one per visit (kernels3.cu:3356-3395:
    pairs inside no_rep, repeats x unique bins, pairs of repeats, the repeats' diagonal pixels)."""
    pix = lambda a, b: max(a, b) * (max(a, b) - 1) // 2 + min(a, b)
    idx = [pix(int(no_rep[x]), int(no_rep[y])) for y in range(len(no_rep)) for x in range(y)]
    idx += [pix(int(r), int(u)) for r in reps for u in uniq]
    idx += [pix(int(reps[x]), int(reps[y])) for y in range(len(reps)) for x in range(y)]
    idx += [n_bins * (n_bins - 1) // 2 + int(r) for r in reps]
    return np.asarray(idx, dtype=np.int64)


def n_restricted_pixels(no_rep, reps, uniq):
    """Number of pixels sub_compute_likelihood visits (cuda_lib_gl.py:2477-2483)."""
    a, r = len(no_rep), len(reps)
    return a * (a - 1) // 2 + r * len(uniq) + r * (r - 1) // 2 + r


# -- what is computed per case: by the live tests over both kernel classes, by tests/golden/make_ref_fixtures.py over the
# -- reference's kernels, and by the fixture tests over the oracle ------------------------------------------------------------
N_OPS = 13
OPS_NEEDING_FB = (2, 3, 4, 5, 6, 7, 9, 10, 11, 12)   # with fA == fB the engine documents a no-op for these


def mutation_record(D, lay, fA, fB):
    """The 13 candidates of (fA, fB) over kernel class D.  Returns out int32[13, 14, n] (SENTINEL where the last kernel
    wrote nothing), written bool[13, n], stale int32[13] and the pop_id_contigs / split_id_contigs vectors."""
    from tests import util
    s, n = lay["state"], len(lay["state"]["pos"])
    out = np.zeros((N_OPS, len(O.FIELDS), n), np.int32)
    written = np.zeros((N_OPS, n), bool)
    stale = np.zeros(N_OPS, np.int32)
    ids = []
    for op in range(N_OPS):
        cand, n_stale, id_vectors = util.kernel_candidate(D, s, fA, fB, op, lay["max_id"], fill=SENTINEL)
        for i, k in enumerate(O.FIELDS):
            out[op, i] = cand[k]
        written[op] = np.all(out[op] != SENTINEL, axis=0)
        assert np.array_equal(written[op], np.any(out[op] != SENTINEL, axis=0)), "an entry is written whole or not at all"
        stale[op] = n_stale
        ids.append(id_vectors)
    return out, written, stale, ids


def state_of(out_op):
    return {k: np.ascontiguousarray(out_op[i]) for i, k in enumerate(O.FIELDS)}


def likelihood_record(dev, lay):
    """(per-pixel float64[n_pix], total) of the layout's full evaluation over the kernels `dev`."""
    per_pix = np.zeros(dev.n_pix, np.float64)
    total = dev.evaluate(lay["state"], per_pix)
    return per_pix, total


def delta_record(dev, D, lay, per_pix, fA, fBs):
    """sub_compute_likelihood of the 13 candidates of every neighbour: float64[K, 13], NaN where the candidate is stale (the
    kernel left entries unwritten, so the reference's value depends on what its slot held before).  Also returns the
    summation-order bound of every entry: N * 2^-53 * sum |term| over the N pixels visited, old and new value of each
    pixel counted as terms."""
    from tests import util
    s = lay["state"]
    deltas = np.full((len(fBs), N_OPS), np.nan)
    bounds = np.zeros((len(fBs), N_OPS))
    for k, fB in enumerate(fBs):
        no_rep, reps, uniq = pixel_lists(lay, s, fA, fB)
        for op in range(N_OPS):
            cand, n_stale, _ = util.kernel_candidate(D, s, fA, fB, op, lay["max_id"], fill=SENTINEL)
            if n_stale:
                continue
            deltas[k, op] = dev.sub_compute(cand, no_rep, reps, uniq, per_pix)
            new_pix = np.zeros(dev.n_pix, np.float64)
            dev.evaluate(cand, new_pix)
            idx = restricted_pixels(dev.n_bins, no_rep, reps, uniq)
            assert len(idx) == n_restricted_pixels(no_rep, reps, uniq)
            bounds[k, op] = 2 * len(idx) * 2.0 ** -53 * (np.abs(new_pix[idx]).sum() + np.abs(per_pix[idx]).sum())
    return deltas, bounds


# -- the recorded fixtures: tests/golden/ref_mutations.npz and ref_likelihood.npz ---------------------------------------------
# Numbers only, inputs regenerated from the seeds above and guarded by `digest`.  Candidate layouts are stored as the
# difference to the input layout on the entries the last kernel wrote (zero elsewhere; the mask is stored next to it):
# lossless, and what makes 81 x 13 candidate layouts fit the size limit of a committed file.
def fixture_arrays(D):
    """(mutations, likelihood): the two fixtures' arrays, computed over kernel class D."""
    mut = {"digest": np.array([lay["digest"] for lay in LAYOUTS], np.int64)}
    lik = {"digest": mut["digest"].copy()}
    for li, lay in enumerate(LAYOUTS):
        s = lay["state"]
        base = np.stack([s[k] for k in O.FIELDS]).astype(np.int32)
        pairs = [(fA, fB) for fA, fBs in lay["proposals"] for fB in fBs]
        diffs, masks, stales = [], [], []
        for fA, fB in pairs:
            out, written, stale, _ = mutation_record(D, lay, fA, fB)
            diffs.append(np.where(written[:, None, :], out - base[None], 0).astype(np.int32))
            masks.append(written)
            stales.append(stale)
        mut["l%d_diff" % li] = np.stack(diffs)
        mut["l%d_written" % li] = np.packbits(np.stack(masks), axis=-1)
        mut["l%d_stale" % li] = np.stack(stales)
        dev = kernels_for(lay, D)
        per_pix, total = likelihood_record(dev, lay)
        lik["l%d_pixels" % li] = per_pix
        lik["l%d_total" % li] = np.float64(total)
        lik["l%d_deltas" % li] = np.stack([delta_record(dev, D, lay, per_pix, fA, fBs)[0] for fA, fBs in lay["proposals"]])
    return mut, lik


# -- the same under the parameter sets of tests/param_cases.py: tests/golden/ref_likelihood_params.npz ------------------------------
# Four layouts (generic and grid coordinates, rings, mixed RF counts, repeated bins) x every set; the layouts, the proposals and the
# contacts are the ones above, only param_simu differs -- so the candidates' layouts are ref_mutations.npz's.  Totals and deltas only:
# the per-pixel vectors are left out to keep the file small (the live tests compare them).
PARAM_LAYOUTS = ("lin_3sub_mixed_generic", "circ_1sub_generic", "circ_3sub_mixed_generic", "rep_3sub_uniform_grid")
PARAM_LAYOUT_INDEX = tuple([lay["name"] for lay in LAYOUTS].index(n) for n in PARAM_LAYOUTS)


def layout_under(li, name):
    """Layout li under the parameter set `name` (its own fact and v_inter, d_max by bisection as for the layout itself), digest included."""
    from tests import param_cases
    lay = LAYOUTS[li]
    P = param_cases.with_params(lay["P"], name)
    return dict(lay, P=P, params=name, digest=_digest(P, lay["state"]))


def param_key(li, name, what):
    return "l%d_%s_%s" % (li, name, what)


def param_fixture_arrays(D):
    """The arrays of ref_likelihood_params.npz, computed over kernel class D."""
    from tests import param_cases
    out = {}
    for li in PARAM_LAYOUT_INDEX:
        for name in param_cases.NAMES:
            lay = layout_under(li, name)
            dev = kernels_for(lay, D)
            per_pix, total = likelihood_record(dev, lay)
            out[param_key(li, name, "digest")] = np.int64(lay["digest"])
            out[param_key(li, name, "total")] = np.float64(total)
            out[param_key(li, name, "deltas")] = np.stack([delta_record(dev, D, lay, per_pix, fA, fBs)[0] for fA, fBs in lay["proposals"]])
    return out


def recorded_candidates(mut, li):
    """Decode ref_mutations.npz for layout li: (out int32[pairs, 13, 14, n] with SENTINEL on unwritten entries,
    written bool[pairs, 13, n], stale int32[pairs, 13]); refuses inputs that drifted from the recorded ones."""
    lay = LAYOUTS[li]
    assert int(mut["digest"][li]) == lay["digest"], "the regenerated inputs of %s are not the recorded ones" % lay["name"]
    n = len(lay["state"]["pos"])
    base = np.stack([lay["state"][k] for k in O.FIELDS]).astype(np.int32)
    written = np.unpackbits(mut["l%d_written" % li], axis=-1)[..., :n].astype(bool)
    out = np.where(written[:, :, None, :], mut["l%d_diff" % li] + base[None, None], SENTINEL).astype(np.int32)
    return out, written, mut["l%d_stale" % li]
