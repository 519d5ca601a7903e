"""GPU: the hand-offs behind the tables of a short-contig step -- table blocks -> the finishing block of k_tm -> the host.

The finishing block reads tables that OTHER blocks of the same launch wrote, and they are rewritten EVERY step: what a missing release,
acquire or wait shows is a table of an EARLIER step, read from a cache that is warm.  One evaluation on a fresh engine cannot see that.  So
every test here runs its evaluations back to back on ONE engine and compares EVERY one of them -- all K x 13 values, as 64-bit words --
with a second engine on the same layout whose table kernel never finishes a step (set_finisher(0)): there k_fin or the reference
arithmetic's kernels finish, launched by the host behind a hand-off of their own.

* soak, idle chip: 2,000 bins, 100,000 contacts, the exploded layout plus 300 MCMC steps (contigs of 1-7 fragments), 4,000 proposals drawn
  like bench.py's; K = 1 (one table block, nothing handed over: the control), 2, 5 and 10 (the largest hand-off); both arithmetics; once
  with three sub-fragments per bin and mixed RF counts;
* soak, loaded chip: the same beside a streaming pass over 2,200,000 contacts (set_scan_path(1): blocks of 1,024 threads on every CU while the
  finishing block polls), K = 5 and 10, reference arithmetic; every step streamed and every step was finished by k_tm;
* hand-backs: the smallest layouts that make the finishing block give the step back -- a neighbour whose set has 21 fragments (the early
  word, no wait) and sets of 20 fragments that queue more than 64 contacts (the word behind the wait) --, where the kernels launched
  afterwards read the tables through the per-neighbour completion words."""
import numpy as np
import pytest

from graal_amd import synth
from tests.test_scan_rows_gpu import engine_for, layout_of_groups, make, map_neighbours, numpy_count, set_arithmetic

pytestmark = pytest.mark.gpu

N_EVALS = 4000
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for S in _cache.values():
        S["ref"].close()
        S["smp"].free_gpu()
    _cache.clear()


def soak_setup(n_sub, which, n_bins, nnz, mcmc_steps, seed):
    """(sampler, reference engine, max_id of each, proposals per K): the sampler's engine after `mcmc_steps` real steps from the exploded
    layout, and a second engine holding the very same layout whose table kernel never finishes a step.  Built once per configuration."""
    key = (n_sub, which, n_bins, nnz, mcmc_steps, seed)
    if key in _cache:
        return _cache[key]
    import bench
    P = synth.make_problem(n_bins=n_bins, nnz=nnz, n_sub=n_sub, seed=seed, accu=1 if n_sub == 1 else ("random", 3, 12))
    P["S_o_A_frags"] = bench.exploded_layout(P)
    rng = np.random.RandomState(seed)
    smp = bench.build_sampler(P, rng, None, 0, which)
    smp.init_likelihood()
    order = np.arange(P["n_frags"], dtype=np.int32)
    rng.shuffle(order)
    for i in order[:mcmc_steps]:
        smp.step_max_likelihood(int(i), 5)
    max_id = int(smp.modify_gl_cuda_buffer(0))
    state = smp.engine.download_frags()
    lens = np.bincount(state["id_c"])
    print("contigs by length:", np.bincount(lens).tolist())
    assert mcmc_steps < 200 or np.count_nonzero(lens >= 2) >= 20        # the steps did join fragments: not every contig is a single one
    ref = engine_for(P, state)
    set_arithmetic(ref, which)
    ref.set_finisher(0)
    ref_max_id = ref.relabel_contigs()
    smp.engine.set_timing(0)
    out = _cache[key] = dict(P=P, smp=smp, ref=ref, max_id=max_id, ref_max_id=ref_max_id, rng=rng, props={}, state=state)
    return out


def proposals(S, K, max_frags=None):
    """N_EVALS proposals drawn like bench.py's: a uniform fragment, up to K neighbours from its row of the contact map, sorted.
    max_frags: only proposals whose contigs hold at most so many fragments in all."""
    if (K, max_frags) not in S["props"]:
        id_c, l_cont = S["state"]["id_c"], S["state"]["l_cont"]
        props = []
        while len(props) < N_EVALS:
            f = int(S["rng"].randint(0, S["P"]["n_frags"]))
            nb = S["smp"].return_neighbours(f, K)
            nb.sort()
            if not len(nb):
                continue
            if max_frags is not None:
                _, one = np.unique(id_c[[f] + list(nb)], return_index=True)     # one fragment of every contig
                if int(l_cont[np.asarray([f] + list(nb))[one]].sum()) > max_frags:
                    continue
            props.append((f, np.asarray(nb, np.int32)))
        S["props"][(K, max_frags)] = props
    return S["props"][(K, max_frags)]


def soak(S, K, scan_path=0, max_frags=None):
    """Every proposal on the engine under test, back to back; then on the reference engine; every value compared."""
    e, ref = S["smp"].engine, S["ref"]
    props = proposals(S, K, max_frags)
    assert max(len(nb) for _, nb in props) == K
    e.set_scan_path(scan_path)
    before = e.run_counters()
    got = [e.eval_candidates(f, nb, S["max_id"]) for f, nb in props]
    after = e.run_counters()
    e.set_scan_path(0)
    want = [ref.eval_candidates(f, nb, S["ref_max_id"]) for f, nb in props]
    grown = {k: after[k] - before[k] for k in after}
    print("K = %d: %d evaluations, %d handed to a finishing kernel, %d indexed, %d fallbacks, %d give-ups" %
          (K, grown["evaluations"], grown["handed_to_a_finishing_kernel"], grown["indexed_passes"], grown["fallbacks"], grown["finisher_gave_up"]))
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if not np.array_equal(a.view(np.int64), b.view(np.int64))]
    assert not bad, (K, len(bad), bad[:10], props[bad[0]], got[bad[0]], want[bad[0]])
    assert any(np.abs(np.nan_to_num(b)).max() > 0 for b in want)
    # (a give-up -- the bounded wait for the scan ran out, 50 us: the host was late with the second launch -- is a hand-over like any other
    # and is printed above, not asserted on)
    assert grown["evaluations"] == len(props) and grown["fallbacks"] == 0
    return grown


@pytest.mark.parametrize("K", [1, 2, 5, 10])
@pytest.mark.parametrize("which", ["strict", "exact"])
def test_soak_idle_chip(which, K):
    S = soak_setup(1, which, 2000, 100000, 300, 20141217)
    grown = soak(S, K)
    # the test is about the finishing block: thousands of these steps must be its own (it gives a step back when the scan queued more than 64
    # contacts or a neighbour's mass work is too large for its table block, which proposals among contigs of several fragments do)
    assert N_EVALS - grown["handed_to_a_finishing_kernel"] >= 1000


def test_soak_idle_chip_three_sub_fragments_mixed_rf_counts():
    S = soak_setup(3, "strict", 2000, 100000, 300, 20141218)
    grown = soak(S, 5)
    assert N_EVALS - grown["handed_to_a_finishing_kernel"] >= 1000


@pytest.mark.parametrize("K", [5, 10])
def test_soak_beside_a_streaming_pass(K):
    """20,000 bins, 2,200,000 contacts, 100 MCMC steps.  The finishing block keeps a step whose scan queued at most 64 contacts; a proposal
    whose contigs hold at most 11 fragments in all (K = 10: fA and ten single fragments) cannot queue more than their 55 pairs, so only such
    proposals are drawn here -- neighbours come from fA's row of the contact map, they are neighbours of each other too, and twelve fragments
    do queue 66."""
    S = soak_setup(1, "strict", 20000, 2_200_000, 100, 20141219)
    assert len(S["P"]["coo_row"]) >= 2_000_000
    grown = soak(S, K, scan_path=1, max_frags=11)
    assert grown["indexed_passes"] == 0                        # every step streamed the list ...
    assert grown["handed_to_a_finishing_kernel"] == 0          # ... and k_tm's last block finished it


# ---- hand-backs ---------------------------------------------------------------------------------------------------------------------------

def hand_back_case(P, state, evals, plain, coo=None, rounds=1):
    """`evals` x `rounds` on an engine under test and on the reference engine: every one equal, every one handed to a finishing kernel.
    Each is followed by two of `plain` -- steps the table kernel finishes itself: in reference arithmetic the host keeps a running mean of
    "this step needed more than k_tm" (weight 1/10) and above 1/2, i.e. from the 7th such step in a row, launches the finishing kernel with
    every step and k_tm no longer publishes; one step in three keeps the mean below 0.37, so every hand-back here is k_tm's own.  (The tables
    the later kernels read are then rewritten between two hand-backs by steps of the other flow as well.)"""
    e, ref = engine_for(P, state, coo), engine_for(P, state, coo)
    for x in (e, ref):
        set_arithmetic(x, "strict")
    ref.set_finisher(0)
    m, mr = e.relabel_contigs(), ref.relabel_contigs()
    seq = []
    for j, ev in enumerate(evals * rounds):
        seq += [ev, plain[(2 * j) % len(plain)], plain[(2 * j + 1) % len(plain)]]
    before = e.run_counters()
    got = [e.eval_candidates(f, nb, m) for f, nb in seq]
    after = e.run_counters()
    want = [ref.eval_candidates(f, nb, mr) for f, nb in seq]
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if not np.array_equal(a.view(np.int64), b.view(np.int64))]
    assert not bad, (len(bad), bad[:10], seq[bad[0]])
    assert any(np.abs(np.nan_to_num(b)).max() > 0 for b in want[::3]) and any(np.abs(np.nan_to_num(b)).max() > 0 for b in want[1::3])
    print("%d evaluations, %d handed to a finishing kernel, %d give-ups" % (len(seq), after["handed_to_a_finishing_kernel"] - before["handed_to_a_finishing_kernel"],
                                                                          after["finisher_gave_up"] - before["finisher_gave_up"]))
    # every hand-back, and nothing else but a step whose bounded wait for the scan ran out (the host late with the second launch)
    handed = after["handed_to_a_finishing_kernel"] - before["handed_to_a_finishing_kernel"]
    assert len(evals) * rounds <= handed <= len(evals) * rounds + after["finisher_gave_up"] - before["finisher_gave_up"]
    assert after["fallbacks"] == before["fallbacks"] == 0
    e.close()
    ref.close()


def plain_steps(P, s, rng, frags, avoid, k):
    """Steps the table kernel finishes itself: fA from `frags`, up to k neighbours from its row of the map outside `avoid`, contigs of at most 4
    fragments -- at most 4 (k + 1) fragments in all; at k = 1 their 28 pairs cannot queue more than the 64 contacts the finishing block takes."""
    out = []
    for fA in frags:
        nb = np.asarray([int(x) for x in map_neighbours(P, int(fA), k + 2, rng) if x not in avoid][:k], np.int32)
        if len(nb) and s["l_cont"][int(fA)] <= 4 and max(s["l_cont"][nb]) <= 4:
            out.append((int(fA), nb))
    assert len(out) >= 4
    return out


def test_hand_back_for_a_set_of_21_fragments_next_to_inline_neighbours():
    """fA alone in its contig, one neighbour in a contig of 20 fragments (a set of 21: one past what the table block prices itself), the other
    neighbours in contigs of at most 4: the last table block says so at once, without waiting for the scan."""
    P = make(1, 91, 400, 30000)
    rng = np.random.RandomState(91)
    ids = rng.permutation(P["n_frags"])
    big, singles = ids[:20], ids[20:32]
    s = layout_of_groups(P, rng, [big] + [singles[i:i + 1] for i in range(len(singles))], rest_max=4)
    evals = []
    for fA in singles:
        others = [int(x) for x in map_neighbours(P, int(fA), 3, rng) if x not in big]
        nb = np.unique(np.asarray(others + [int(rng.choice(big))], np.int32))
        assert s["l_cont"][int(fA)] == 1 and max(s["l_cont"][nb]) == 20 and len(nb) >= 2
        evals.append((int(fA), nb))
    plain = plain_steps(P, s, rng, singles, set(int(x) for x in big), 1)
    hand_back_case(P, s, evals, plain, rounds=25)      # 300 hand-backs among 900 evaluations


def test_hand_back_behind_the_wait_when_sets_of_20_queue_more_than_64_contacts():
    """Two contigs of 10 fragments with every pair of their 20 fragments in contact (190 contacts): each set is small enough for the table
    blocks, the queue is not for the finishing block -- it gives the step back behind its wait for the scan."""
    P = make(1, 92, 400, 30000)
    rng = np.random.RandomState(92)
    ids = rng.permutation(P["n_frags"])
    g1, g2 = ids[:10], ids[10:20]
    both = np.sort(ids[:20])
    assert np.array_equal(P["bin_of_sub"], np.arange(P["n_frags"]))     # one sub-fragment per bin: a contact's ids are its bins
    ii, jj = np.triu_indices(20, 1)
    row = np.concatenate([P["coo_row"], both[ii].astype(P["coo_row"].dtype)])
    col = np.concatenate([P["coo_col"], both[jj].astype(P["coo_col"].dtype)])
    val = np.concatenate([P["coo_val"], np.full(len(ii), 3, P["coo_val"].dtype)])
    n = int(P["init_n_sub_frags"])
    _, first = np.unique(row.astype(np.int64) * n + col, return_index=True)   # (sorted by row, then col; a pair listed once)
    row, col, val = row[first], col[first], val[first]
    s = layout_of_groups(P, rng, [g1, g2], rest_max=4)
    evals = []
    for a, b in zip(g1, g2):
        for fA, fB in ((int(a), int(b)), (int(b), int(a))):
            nb = np.asarray([fB], np.int32)
            assert numpy_count(P, s, fA, nb, row, col) > 64       # on the CPU: the case does queue more than the finishing block takes
            assert s["l_cont"][fA] + s["l_cont"][fB] == 20
            evals.append((fA, nb))
    plain = plain_steps(P, s, rng, ids[20:60], set(int(x) for x in ids[:20]), 1)
    hand_back_case(P, s, evals, plain, coo=(row, col, val), rounds=15)   # 300 hand-backs among 900 evaluations
