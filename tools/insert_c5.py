"""Insertions on a C5-size layout (bench.py's 50,000-fragment / 20 M-contact stand-in).

    python tools/insert_c5.py [--reps N] [--nnz N]      one JSON line per measurement -> profiles/insert_c5.md

The layout: the map in contigs of 80 fragments, a piece of 1-3 fragments cut out of every contig at an interior position (its own contig,
every other one reversed), the contig closed over the gap -- a late-stage layout with small pieces to put back.
  - "insertions": graal_insertions + its fetch at max_piece_frags 1 and 3: ms per call, the listed count, and how many pieces of that
    size have their true insertion listed, as their best, and as a mutual pair;
  - "yardsticks": a full evaluation and graal_end_links_best (min_frags 1) on the same layout, ms per call;
  - "insert_round": the round's plan at max_piece_frags 1 (plan_insertions) applied by graal_edit_layout, ms per call (the layout is
    uploaded again between calls, outside the timing), the logL before and after, and the kept rows' scores and their sum.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def cut_layout(P, k, seed=1):
    """(layout, truth): truth[piece head] = (the fragment before its gap, the rev that puts it back as it was)."""
    from tests.link_reference import contig_lists, layout
    from tools.junctions_c5 import chopped
    s = chopped(P, k)
    rng = np.random.RandomState(seed)
    contigs, pieces, truth = [], [], {}
    for c, frags in contig_lists(s).items():
        if len(frags) < 20:
            contigs.append(frags)
            continue
        w = int(rng.randint(1, 4))
        at = int(rng.randint(5, len(frags) - 5 - w))
        piece = frags[at:at + w]
        rev = len(pieces) % 2
        if rev:
            piece = [(x, -o) for x, o in reversed(piece)]
        truth[int(piece[0][0])] = (int(frags[at - 1][0]), rev)
        pieces.append(piece)
        contigs.append(frags[:at] + frags[at + w:])
    return layout(s["len_bp"], contigs + pieces), truth


def truth_stats(t, truth, max_frags, lc):
    """How many pieces of <= max_frags fragments have their true insertion listed, as their best, and as a mutual pair."""
    from graal_amd import insert
    p, f, r = (np.asarray(t[k]) for k in ("piece", "after", "rev"))
    row = {(int(a), int(b), int(c)): i for i, (a, b, c) in enumerate(zip(p, f, r))}
    by_piece, by_junction = insert.best_insertions(t)
    mutual = set(insert.mutual_insertions(t).tolist())
    n = listed = best = mut = 0
    for head, (ft, rv) in truth.items():
        if lc[head] > max_frags:
            continue
        n += 1
        i = row.get((head, ft, rv))
        if i is None:
            continue
        listed += 1
        best += by_piece.get(head) == i
        mut += i in mutual
    return {"pieces": n, "true_listed": listed, "true_best": best, "true_mutual": mut}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--nnz", type=int, default=20_000_000)
    args = ap.parse_args()
    from graal_amd import insert, synth
    from graal_amd.lib import Engine, GraalError
    from tools.scaffold_c5 import timed
    P = synth.make_problem(n_bins=50000, nnz=args.nnz, n_sub=1, seed=20141217)
    e = Engine(0)
    try:
        e.upload_subfrags(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["init_n_sub_frags"],
                          P["mean_squared_frags_per_bin"])
        e.upload_contacts(P["coo_row"], P["coo_col"], P["coo_val"])
        e.set_params(P["param_simu"])
        s, truth = cut_layout(P, 80)
        n_pieces = len(truth)
        e.upload_frags(s)
        e.relabel_contigs()
        s = e.download_frags()
        for mf in (1, 3):
            try:
                ms = timed(lambda: e.insertions_q(mf), args.reps)
            except GraalError as err:
                print(json.dumps({"measure": "insertions", "max_piece_frags": mf, "refused": str(err)}), flush=True)
                continue
            t = insert.insertion_table(e, mf)
            print(json.dumps({"measure": "insertions", "fragments": int(len(s["pos"])), "contacts": int(len(P["coo_row"])),
                              "pieces": n_pieces, "max_piece_frags": mf, "listed": int(len(t["score"])),
                              "valid": int(np.isfinite(t["score"]).sum()), "insertions_ms": ms,
                              **truth_stats(t, truth, mf, s["l_cont"])}), flush=True)
        full = timed(lambda: e.eval_full(), args.reps)
        best = timed(lambda: e.end_links_best(1), args.reps)
        print(json.dumps({"measure": "yardsticks", "eval_full_ms": full, "end_links_best_ms": best}), flush=True)
        t = insert.insertion_table(e, 1)
        cuts, joins, kept = insert.plan_insertions(t, s, 0.0)
        ed = timed(lambda: e.edit_layout(cuts, joins), args.reps, before=lambda: e.upload_frags(s))
        e.upload_frags(s)
        e.relabel_contigs()
        logl0 = e.eval_full()
        e.edit_layout(cuts, joins)
        e.relabel_contigs()
        logl1 = e.eval_full()
        print(json.dumps({"measure": "insert_round", "insertions": int(len(kept)), "edit_layout_ms": ed, "logL_before": logl0,
                          "logL_after": logl1, "logL_delta": logl1 - logl0, "kept_scores": [float(x) for x in t["score"][kept]],
                          "kept_score_sum": float(np.sum(t["score"][kept]))}), flush=True)
    finally:
        e.close()


if __name__ == "__main__":
    main()
