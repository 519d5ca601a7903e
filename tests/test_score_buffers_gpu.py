"""The whole-layout scorers (graal_junction_scores, graal_junction_bootstrap, graal_junction_gaps, graal_ring_scores, graal_layout_maps,
graal_end_links, graal_end_links_best, graal_insertions) keep their buffers on the handle between calls: the slots and the layout records (one set per family, each built on
layout_slots.h's LayoutSlots) are reallocated when (n, S) changes, the candidate table, the maps' image buffers and the hipCUB scratch
grow to the largest size a call needed and are then used at a smaller size than their allocation.  Every call on a handle that served other calls
must return exactly what the same call returns as the FIRST call on a fresh handle with the same uploads.  Nothing here is compared with
stored numbers: the other GPU tests tie the fresh-handle results to the numpy restatements; here the restatements only show, before any
launch, that the ring scores are not all zero (at least 10 contigs with a non-zero score in the cut layouts, all 3 in the uncut ones),
and the first maps call must see contacts (a non-zero observed image), so that a buffer left all zero cannot pass.  The bootstrap and
the gap profile fill ONE batch pair of the junction scorer's buffers (rows * n each, grown to the largest call): their fresh results
must score at least 10 junctions, with a non-zero replicate matrix and a non-zero profile row beyond gap 0.

Problem A is window_cases.small_cut("w3") under ref_trans_accu: 160 bins at n_sub 3 with mixed RF counts (the mirror sums, both quirk
kernels and the insertions' second table are live), pieces of 1-4 and 25-60 bins.  Problem B is small_cut("w1"): 240 fragments at n_sub
1, the quirk off.  The uncut layouts have the same n and far fewer contigs: the tables shrink in use, not in allocation.  The last test
loads problem B into a handle that served problem A (a second upload_subfrags / upload_contacts / upload_frags on a live handle is
accepted), so the records are reallocated for another (n, S)."""
import numpy as np
import pytest

from graal_amd.lib import JUNCTION_VALID
from tests import junction_gap_reference as GR
from tests import ring_reference as RR
from tests import window_cases
from tests.test_scaffold_gpu import engine_for

pytestmark = pytest.mark.gpu

QUIRK = {"w3": True, "w1": False}


def grid(e):
    """GR.small_grid (11 gap values) of the problem the engine holds, A or B, told apart by their sizes."""
    return GR.small_grid(problem({160: "w3", 240: "w1"}[int(e.n)])[0])


CALLS = {
    "links1": lambda e: e.end_links_q(1),
    "links3": lambda e: e.end_links_q(3),
    "best1": lambda e: e.end_links_best(1),
    "best3": lambda e: e.end_links_best(3),
    "ins1": lambda e: e.insertions_q(1),
    "ins4": lambda e: e.insertions_q(4),
    "junctions": lambda e: e.junction_scores_q(),
    "rings": lambda e: e.ring_scores_q(),
    "maps64": lambda e: e.layout_maps(64)[:4],     # (the three images and pixel_of_sub)
    "maps4096": lambda e: e.layout_maps(4096)[:4],
    "boot3": lambda e: e.junction_bootstrap_q(1, 3, 0, replicates=True),
    "boot20": lambda e: e.junction_bootstrap_q(1, 20, 0),
    "gaps11": lambda e: e.junction_gaps_q(grid(e), GR.DROP_Q, profile=True),
    "gaps3": lambda e: e.junction_gaps_q(grid(e)[[0, 5, 9]], GR.DROP_Q, profile=True),
}
# links1 after links3: the table grows; links3 after it: the allocation is larger than the `cap` in use.  maps4096 after maps64: the image
# buffers grow; maps64 after it: they are used small.  rings and the maps each follow a call of another family.  boot3, gaps11, boot20: the
# batch pair the bootstrap and the gaps share grows three times; gaps3: it is used smaller than its allocation; then junctions and rings,
# and boot3 takes it over from the gaps; the last gaps11 takes it back
SEQUENCE = ("links3", "maps64", "boot3", "best1", "rings", "gaps11", "links1", "maps4096", "boot20", "links3", "gaps3", "ins4", "maps64",
            "ins1", "junctions", "rings", "boot3", "best3", "maps4096", "gaps11")
UNCUT = ("links1", "rings", "gaps3", "best1", "maps64", "boot20", "ins4", "maps4096", "junctions", "rings", "gaps11", "boot3")

_PROBLEMS, _FRESH = {}, {}


def problem(name):
    if name not in _PROBLEMS:
        _PROBLEMS[name] = (window_cases.small_cut(name), window_cases.small(name)["S_o_A_frags"])
    return _PROBLEMS[name]


def flat(result):
    if isinstance(result, dict):                      # (the bootstrap and the gaps: their arrays in key order)
        result = tuple(result[k] for k in sorted(result))
    out = []
    for x in result:
        out.extend(flat(x) if isinstance(x, (tuple, dict)) else [np.asarray(x)])
    return out


def fresh_result(name, layout, call):
    """`call` as the first call on a fresh handle loaded with problem `name` in layout 'cut' or 'uncut' (computed once)."""
    key = (name, layout, call)
    if key not in _FRESH:
        P, uncut = problem(name)
        e = engine_for(P, state=uncut if layout == "uncut" else None, quirk=QUIRK[name])
        try:
            _FRESH[key] = CALLS[call](e)
        finally:
            e.close()
    return _FRESH[key]


def fresh(name, layout, call):
    return flat(fresh_result(name, layout, call))


def check(e, name, layout, call, step):
    got, want = flat(CALLS[call](e)), fresh(name, layout, call)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and np.array_equal(g, w), (name, layout, call, step, i)


def assert_rings_and_maps_score(name, layout):
    """Rings, on the CPU: enough contigs with a non-zero score.  Maps: the fresh handle's observed images are not empty."""
    P, uncut = problem(name)
    state = uncut if layout == "uncut" else P["S_o_A_frags"]
    R = RR.ring_scores_windowed(P, state=state)[0]
    idc = np.asarray(state["id_c"])
    scoring, contigs = len(set(idc[R != 0].tolist())), len(set(idc.tolist()))
    if layout == "cut":
        assert scoring >= 10, (name, layout, scoring)
    else:
        assert scoring == contigs == 3, (name, layout, scoring, contigs)
    for call in ("maps64", "maps4096"):
        assert fresh(name, layout, call)[0].astype(np.float64).sum() != 0, (name, layout, call)
    assert fresh(name, layout, "maps4096")[0].size > fresh(name, layout, "maps64")[0].size


def assert_rows_score(name, layout):
    """The bootstrap and the gaps, on fresh handles: enough scored junctions, replicates and profile rows that are not all zero."""
    for call, matrix in (("boot3", "q_rep"), ("boot20", None), ("gaps11", "q_gap"), ("gaps3", "q_gap")):
        t = fresh_result(name, layout, call)
        assert (t["status"] == JUNCTION_VALID).sum() >= 10, (name, layout, call)
        if matrix == "q_rep":
            assert t[matrix].shape[0] == 3 and t[matrix].any(), (name, layout, call)
        elif matrix == "q_gap":
            assert t[matrix][1:].any(), (name, layout, call)
        else:
            assert t["q_sum"].any() and t["support"].any(), (name, layout, call)
    assert fresh_result(name, layout, "gaps11")["q_gap"].shape[0] == 11 and fresh_result(name, layout, "gaps3")["q_gap"].shape[0] == 3


@pytest.mark.parametrize("name", ["w3", "w1"])
def test_reused_handle_equals_fresh_handle(name):
    P, uncut = problem(name)
    assert_rings_and_maps_score(name, "cut")
    assert_rings_and_maps_score(name, "uncut")
    assert_rows_score(name, "cut")
    assert_rows_score(name, "uncut")
    assert len(fresh(name, "cut", "links1")[0]) > len(fresh(name, "cut", "links3")[0]) > len(fresh(name, "uncut", "links1")[0]) > 0
    assert len(fresh(name, "cut", "ins4")[0]) > len(fresh(name, "cut", "ins1")[0]) > 0
    e = engine_for(P, quirk=QUIRK[name])
    try:
        for step, call in enumerate(SEQUENCE):
            check(e, name, "cut", call, step)
        e.upload_frags(uncut)
        for step, call in enumerate(UNCUT):
            check(e, name, "uncut", call, len(SEQUENCE) + step)
    finally:
        e.close()


def test_another_problem_on_a_used_handle():
    A, _ = problem("w3")
    B, _ = problem("w1")
    assert len(A["S_o_A_frags"]["pos"]) != len(B["S_o_A_frags"]["pos"])
    first = ("links1", "maps4096", "best1", "rings", "boot20", "ins4", "junctions", "gaps3")
    second = ("rings", "gaps11", "links1", "maps64", "best1", "boot3", "ins4", "maps4096", "junctions", "rings", "links3", "gaps3", "maps64",
              "boot20")
    assert_rings_and_maps_score("w3", "cut")
    assert_rings_and_maps_score("w1", "cut")
    assert_rows_score("w3", "cut")
    assert_rows_score("w1", "cut")
    e = engine_for(A, quirk=True)
    try:
        for step, call in enumerate(first):
            check(e, "w3", "cut", call, step)
        e.upload_subfrags(B["np_sub_frags_id"], B["np_sub_frags_len_bp"], B["np_sub_frags_accu"], B["init_n_sub_frags"],
                          B["mean_squared_frags_per_bin"])
        e.upload_contacts(B["coo_row"], B["coo_col"], B["coo_val"])
        e.set_params(B["param_simu"])
        e.upload_frags(B["S_o_A_frags"])
        e.set_mode(ref_trans_accu=False)
        for step, call in enumerate(second):
            check(e, "w1", "cut", call, len(first) + step)
    finally:
        e.close()
