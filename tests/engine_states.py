"""TEST INFRASTRUCTURE -- engines for the mid-size GPU tests (tests/test_layout_scores_midsize_gpu.py, tests/test_maps_midsize_gpu.py) in
the states that decide how graal_junction_scores and graal_layout_maps are launched, the rule by which the handle sizes those launches,
graal_begin_step's relabel in numpy, and the cache the two modules share their problems and references through.  Not product code.
"""
import numpy as np

from graal_amd.lib import Engine
from tests import link_reference as LR

GRID_CONTACTS = 2048 * 4 * 64           # the contact-streaming kernels' contacts per grid pass

_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


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


def stripes_of(lc, n):
    """k_jn_mass's and k_mp_cis's waves per 64-slot x tile for a layout of n fragments on a handle whose last begin_step saw a longest
    contig of lc (0 on a new handle): junctions.h / maps.h's rule restated, the clamp to n included (it matters only where a stale lc
    exceeds the fragments of the layout scored, which no case here does).  The launch itself cannot be read back: this is the rule
    applied to the statistic the device reported, not an observation of the grid."""
    lc = min(max(int(lc), 1), int(n))
    return min(16, max(1, ((lc + 63) // 64 + 7) // 8))


def relabelled(s):
    """The layout after graal_begin_step's relabel: id_c <- the contig's rank by (l_cont, old label); nothing else moves."""
    out = {k: np.array(v) for k, v in s.items()}
    labs, first = np.unique(out["id_c"], return_index=True)
    rank = {lab: r for r, (_, lab) in enumerate(sorted(zip(out["l_cont"][first].tolist(), labs.tolist())))}
    out["id_c"] = np.array([rank[int(c)] for c in out["id_c"]], dtype=out["id_c"].dtype)
    return out


def engine_in(engine_state, P, layout=None, quirk=False, before=None):
    """(engine, the layout a reference must be built from, Sw: the waves per x tile its junction and map launches use).  The handle sizes
    those launches by the longest contig of its last graal_begin_step, which an upload leaves alone:
    'fresh'    upload only: Sw = 1 whatever the layout;
    'stepped'  upload, then begin_step, as every run does before it scores: the contigs are relabelled (the layout returned is the
               downloaded one), Sw follows the layout's longest contig (stats[4]);
    'stale'    upload of the layout `before`, begin_step, then upload of the layout asked for: Sw follows `before`'s longest contig."""
    s = P["S_o_A_frags"] if layout is None else layout
    if engine_state == "fresh":
        return engine_for(P, s, quirk), s, 1
    e = engine_for(P, s if engine_state == "stepped" else before, quirk)
    try:
        first = s if engine_state == "stepped" else before
        stats, max_id = e.begin_step()
        assert int(stats[4]) == int(np.max(first["l_cont"])) and max_id == len(np.unique(first["id_c"])) - 1
        Sw = stripes_of(stats[4], len(s["id_c"]))
        if engine_state == "stepped":
            s, want = e.download_frags(), relabelled(s)
            for k in LR.FIELDS:
                assert np.array_equal(s[k], want[k]), k
        else:
            assert engine_state == "stale"
            e.upload_frags(s)
    except BaseException:
        e.close()
        raise
    return e, s, Sw
