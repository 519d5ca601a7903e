"""CPU: the cases of tests/repeat_cases.py are what tests/test_repeats_midsize_gpu.py needs them to be -- checked with the oracle, the
layout and the step plan alone, so that the GPU tests cannot pass for an empty reason: every layout is valid and holds its seven kinds
of placement, the repeated bins' observation rows reach every branch of lik_double and factorial_f, the grids of k_rep_delta and
k_rep_full are many blocks, the plan takes the flow the case is named after, one copy's activity is worth far more than the tolerance,
and a proposal away from every repeated bin owes nothing to their pixels."""
import numpy as np
import pytest

from tests import repeat_cases as RC
from tests import util
from tests.test_step_plan_cpu import flow

CASES = pytest.mark.parametrize("name,variant", RC.CASES)


@CASES
def test_layout_is_valid_and_holds_every_kind_of_placement(name, variant):
    P = RC.problem(name, variant)
    s, max_id = RC.layout(name, variant)
    util.check_invariants(s)
    c = RC.PROBLEMS[name]
    assert len(s["pos"]) == c["n_bins"] + len(c["dup"]) * c["n_extra"] == P["n_new_frags"]
    rep, id_d = s["rep"], s["id_d"]
    n0 = c["n_bins"]
    # what graal_upload_frags asks of the fields, and the issue of the originals
    assert np.all(rep[:n0] == 0) and np.all(s["activ"][:n0] == 1) and np.all(id_d[:n0] == np.arange(n0))
    assert np.all(rep[n0:] == 1) and sorted(set(id_d[n0:].tolist())) == sorted(c["dup"])
    assert np.all(np.bincount(id_d[n0:], minlength=n0)[list(c["dup"])] == c["n_extra"])
    k = RC.layout_kinds(P, s)
    for kind in "abcdefg":
        assert k[kind], kind
    assert len(np.unique(s["id_c"])) == max_id + 1 and s["id_c"].max() == max_id
    # two repeated bins that are neighbours in id, and the last bin, are among the repeated ones
    dup = sorted(c["dup"])
    assert any(b + 1 in dup for b in dup) and dup[-1] == n0 - 1
    assert c["n_extra"] + 1 >= 4                             # copy-pair loops of 4 x 4 and more


@CASES
def test_proposals_are_of_every_kind(name, variant):
    P = RC.problem(name, variant)
    s, _ = RC.layout(name, variant)
    K = RC.PROBLEMS[name]["K"]
    k = RC.layout_kinds(P, s)
    dup = set(RC.PROBLEMS[name]["dup"])
    rep, id_d, id_c, activ = s["rep"], s["id_d"], s["id_c"], s["activ"]
    g_frags = set(f for g in k["g_contigs"] for f in g)
    props = RC.proposals(name, variant)
    assert [p[0] for p in props] == list(RC.PROPOSAL_KINDS)
    for kind, fA, fBs in props:
        assert len(fBs) == K == len(set(fBs)) and fA not in fBs
    (_, f1, _), (_, f2, _), (_, f3, _), (_, f4, _), (_, f5, b5) = props
    assert id_d[f1] not in dup and np.any((id_c == id_c[f1]) & (rep == 1))
    assert rep[f2] == 1 and activ[f2] == 1 and s["l_cont"][f2] == s["l_cont"].max() and 0 < s["pos"][f2] < s["l_cont"][f2] - 1
    assert rep[f3] == 1 and activ[f3] == 0 and s["l_cont"][f3] == 1
    assert rep[f4] == 0 and id_d[f4] in dup and f4 == id_d[f4]
    assert f5 in g_frags and set(b5) <= g_frags
    for kind, fA, fBs in props[:4]:
        b = np.asarray(fBs)
        if id_d[fA] in dup:
            assert np.any((id_d[b] == id_d[fA]) & (rep[b] == 1)), kind                    # a copy of fA's own bin
        assert np.any((id_d[b] != id_d[fA]) & (rep[b] == 1)), kind                        # a copy of another repeated bin
        if s["l_cont"][fA] > 1:
            assert np.any(id_c[b] == id_c[fA]), kind                                      # a fragment of fA's own contig
        assert set(fBs) & g_frags, kind                                                   # a fragment of a contig of kind (g)


@CASES
def test_observation_rows_reach_every_branch_of_the_likelihood(name, variant):
    from tests.test_repeats_gpu import split_observations
    P = RC.problem(name, variant)
    (r, c, v), obs = split_observations(P)
    assert ((obs >= 10) & (obs < 15)).sum() >= 1 and (obs >= 15).sum() >= 1          # factorial_f's Stirling form; lik_double's own
    assert ((obs > 0) & (obs < 10)).sum() >= 1 and (obs == 0).sum() >= 1
    # a count between two repeated bins, and (several sub-fragments) one inside a repeated bin
    ids = np.asarray(P["np_sub_frags_id"]).reshape(-1, 4)
    dup = list(P["id_frag_duplicated"])
    subs = {b: ids[b, :ids[b, 3]] for b in dup}
    assert any(obs[i, a, subs[w]].max() >= 10 for i, b in enumerate(dup) for a in range(len(subs[b])) for w in dup if w != b)
    if RC.PROBLEMS[name]["n_sub"] > 1:
        assert any(obs[i, a, subs[b]].max() >= 10 for i, b in enumerate(dup) for a in range(len(subs[b])))
    # no contact of a repeated bin is left in the list the engine gets
    dup_sub = np.zeros(int(P["init_n_sub_frags"]), bool)
    dup_sub[np.concatenate(list(subs.values()))] = True
    assert not dup_sub[r].any() and not dup_sub[c].any() and len(r) > 0.9 * len(P["coo_row"])


@pytest.mark.parametrize("name", list(RC.PROBLEMS))
def test_grids_are_many_blocks(name):
    c = RC.PROBLEMS[name]
    n_dup, n_bins, K = len(c["dup"]), c["n_bins"], c["K"]
    assert n_dup * n_bins > 256                                # k_rep_full: more than one block
    if name != "late stage":
        assert K == 10 and n_dup * n_bins * K > 256 * 8        # k_rep_delta: every row of s_acc, many blocks
        assert (n_dup * n_bins) % 256 != 0                     # a neighbour's pixels end inside a block


@CASES
def test_plan_takes_the_flow_the_case_is_named_after(name, variant):
    f = RC.plan_facts(name, variant)
    p = flow(**f)
    assert p["rep_delta"] == 1 and p["tm_publishes"] == 0
    assert p["late_stage"] == int(name == "late stage")
    if name == "late stage":
        s, _ = RC.layout(name, variant)
        heads = s["pos"] == 0
        assert (s["l_cont"][heads] > 128).sum() == 2 and f["n_contigs"] == 8
        if variant == "reference":
            assert p["finisher"] == 3                           # the tiled reference-arithmetic kernels


@CASES
def test_oracle_sees_one_copy_and_nothing_where_no_repeat_is(name, variant):
    P, D = RC.problem(name, variant), RC.dense(name, variant)
    s, max_id = RC.layout(name, variant)
    r = RC.oracle_results(name, variant)
    tol = RC.tolerance(variant, r["base"])
    props = RC.proposals(name, variant)
    for (kind, fA, fBs), want in zip(props, r["want"]):
        assert want.shape == (len(fBs), 13) and np.all(np.isfinite(want)), kind
        if s["rep"][fA] == 1:
            assert np.abs(want[:, 8]).min() > 10 * tol, (kind, np.abs(want[:, 8]).min(), tol)
    assert sum(int(s["rep"][fA] == 1) for _k, fA, _b in props) >= 2
    # away from every repeated bin: the reference's list of repeats is empty.  Pricing EVERY repeated pixel under the candidates all the
    # same gives exactly the pixels' current values -- except with the reference's RF-count indexing over several sub-fragments
    # (walk_trans: a reversed bin of lower id is priced with its last sub-fragment's count), where flipping an ordinary bin does move
    # its pixels with the repeated bins; the reference does not look at them then, and a kernel that did would be seen
    kind, fA, fBs = props[4]
    dup = np.asarray(P["id_frag_duplicated"], np.int32)
    uniq = np.setdiff1d(np.arange(P["n_frags"], dtype=np.int32), dup)
    per_pix = np.zeros(D.n_pix)
    D.evaluate(s, per_pix)
    unseen = []
    for k, fB in enumerate(fBs):
        in_ab = np.nonzero((s["id_c"] == s["id_c"][fA]) | (s["id_c"] == s["id_c"][fB]))[0]
        assert len(np.intersect1d(s["id_d"][in_ab], dup)) == 0
        for op in range(13):
            cand, stale = util.oracle_candidate(s, fA, fB, op, max_id)
            assert not stale
            assert D.sub_compute(cand, np.setdiff1d(s["id_d"][in_ab], dup), [], uniq, per_pix) == r["want"][4][k, op]
            unseen.append(D.sub_compute(cand, [], dup, uniq, per_pix))
    if variant == "exact" or RC.PROBLEMS[name]["n_sub"] == 1:
        assert np.all(np.asarray(unseen) == 0.0)
    else:
        assert np.abs(unseen).max() > 10 * tol
    assert np.abs(r["want"][4]).max() > 10 * tol


def test_short_run_of_the_oracle_swaps_an_activity_and_moves_a_copy():
    """What tests/test_repeats_midsize_gpu.py's short run compares against, by itself: the oracle accepts an activity swap (op 8) and
    a move of a copy into or along a contig, and originals and copies of repeated bins are among the fragments stepped.  (The 24 steps
    take the oracle 4 s on the CPU.)"""
    P = RC.problem(RC.RUN["name"], RC.RUN["variant"])
    rep, id_d = P["S_o_A_frags"]["rep"], P["S_o_A_frags"]["id_d"]
    ids = list(RC.RUN["ids"])
    assert len(ids) >= 20
    assert any(rep[i] == 1 for i in ids) and any(rep[i] == 0 and id_d[i] in P["id_frag_duplicated"] for i in ids)
    r = RC.oracle_run()
    assert r["n_stale"] == 0
    assert any(op == 8 and rep[fA] == 1 for fA, _fB, op in r["trace"])
    assert any(2 <= op <= 12 and op != 8 and rep[fA] == 1 for fA, _fB, op in r["trace"])
    assert (r["final"]["activ"] == 0).any()
