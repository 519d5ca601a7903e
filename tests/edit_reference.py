"""TEST INFRASTRUCTURE -- numpy restatement of graal_edit_layout (graal_amd/csrc/edit.h) from the rules of include/graal_hip.h, built on
tests/link_reference.py (layout, contig_lists) and tests/junction_reference.py (cut_layout's field rules).  Not product code.

edit(state, cuts, joins) -> (new state, None) or (None, status) where status holds the refusal codes (graal_amd.lib.EDIT_*)."""
import numpy as np

from graal_amd.lib import (EDIT_BAD_CUT, EDIT_BAD_END, EDIT_CIRCULAR, EDIT_CYCLE, EDIT_DUP_CUT, EDIT_END_TWICE, EDIT_OK,
                           EDIT_SAME_CONTIG)
from tests.link_reference import FIELDS, contig_lists


def _pieces(state, cuts):
    """The contigs after the cuts: {label: (list of (frag, ori), circular, touched)} and the cut statuses."""
    s = {k: np.asarray(v) for k, v in state.items()}
    lists = contig_lists(s)
    st = np.full(len(cuts), EDIT_OK, dtype=np.int32)
    n = len(s["id_c"])
    cutset = {}
    for i, f in enumerate(cuts):
        f = int(f)
        if not 0 <= f < n:
            st[i] = EDIT_BAD_CUT
            continue
        c = int(s["id_c"][f])
        ring = int(s["circ"][f]) == 1
        if (len(lists[c]) < 2) if ring else (int(s["pos"][f]) >= len(lists[c]) - 1):
            st[i] = EDIT_BAD_CUT
            continue
        cutset.setdefault(f, []).append(i)
    for f, idx in cutset.items():
        if len(idx) > 1:
            st[idx] = EDIT_DUP_CUT
    maxlab = int(s["id_c"].max())
    out, fresh = {}, []
    for c, frags in lists.items():
        ring = int(s["circ"][frags[0][0]]) == 1
        at = [k for k, (f, _) in enumerate(frags) if f in cutset]
        if not at:
            out[c] = (frags, ring, False)
            continue
        if ring:      # rotate so that the piece after the last cut comes first: a linear list cut at the other cuts
            r = at[-1] + 1
            order = frags[r:] + frags[:r]
            at = [(k - r) % len(frags) for k in at[:-1]]
        else:
            order = frags
        bounds = [0] + [k + 1 for k in at] + [len(order)]
        parts = [order[bounds[i]:bounds[i + 1]] for i in range(len(bounds) - 1) if bounds[i] < bounds[i + 1]]
        first = frags[0][0]                  # the piece holding position 0 keeps the label
        for p in parts:
            if any(f == first for f, _ in p):
                out[c] = (p, False, True)
            else:
                fresh.append(p)
    for k, p in enumerate(sorted(fresh, key=lambda p: p[0][0])):
        out[maxlab + 1 + k] = (p, False, True)
    return out, st


def edit(state, cuts=(), joins=()):
    s = {k: np.asarray(v) for k, v in state.items()}
    n = len(s["id_c"])
    cuts = [int(x) for x in np.asarray(cuts).reshape(-1)]
    joins = [(int(a), int(b)) for a, b in np.asarray(joins, dtype=np.int64).reshape(-1, 2)]
    pieces, st_cut = _pieces(s, cuts)
    st_join = np.full(len(joins), EDIT_OK, dtype=np.int32)
    end_of = {}                                # end -> label of its piece
    for c, (p, ring, _) in pieces.items():
        end_of[2 * p[0][0]] = (c, ring)
        end_of[2 * p[-1][0] + 1] = (c, ring)
    use = {}
    for j, (a, b) in enumerate(joins):
        code = EDIT_OK
        for e in (a, b):
            if code == EDIT_OK:
                if not 0 <= e < 2 * n or e not in end_of:
                    code = EDIT_BAD_END
                elif end_of[e][1]:
                    code = EDIT_CIRCULAR
        if code == EDIT_OK and end_of[a][0] == end_of[b][0]:
            code = EDIT_SAME_CONTIG
        st_join[j] = code
        if code == EDIT_OK:
            use.setdefault(a, []).append(j); use.setdefault(b, []).append(j)
    for e, js in use.items():
        if len(js) > 1:
            for j in js:
                if st_join[j] == EDIT_OK:
                    st_join[j] = EDIT_END_TWICE
    status = np.concatenate([st_cut, st_join])
    if np.any(status != EDIT_OK):
        return None, status
    partner = {}
    for a, b in joins:
        partner[a] = b; partner[b] = a
    # chains: walk from every piece end; the canonical direction exits the contig of e_min through e_min
    lab_of = {}
    for c, (p, _, _) in pieces.items():
        lab_of[2 * p[0][0]] = c; lab_of[2 * p[-1][0] + 1] = c
    mate = {}
    for c, (p, _, _) in pieces.items():
        mate[2 * p[0][0]] = 2 * p[-1][0] + 1; mate[2 * p[-1][0] + 1] = 2 * p[0][0]
    done, chains = set(), []
    for j, (a, _) in enumerate(joins):
        if lab_of[a] in done:
            continue
        # walk back from a's piece to a terminal, detecting a cycle
        x, seen, cyc = a, set(), False         # x: an end of the current piece; go away from x
        while True:
            c = lab_of[x]
            if c in seen:
                cyc = True
                break
            seen.add(c)
            if x not in partner:
                break
            x = mate[partner[x]]
        if cyc:
            for jj, (aa, bb) in enumerate(joins):
                if lab_of[aa] in seen:
                    st_join[jj] = EDIT_CYCLE
            continue
        start = x                              # a free end of the chain's terminal piece: the walk enters there
        order, z = [], start
        while True:
            order.append((lab_of[z], z))       # (piece, entry end)
            m = mate[z]
            if m not in partner:
                break
            z = partner[m]
        ends = [e for _, z in order for e in (z, mate[z]) if e in partner]
        e_min = min(ends)
        exits = {mate[z] for _, z in order}
        if e_min not in exits:                 # the other direction
            z = mate[order[-1][1]]
            order = []
            while True:
                order.append((lab_of[z], z))
                m = mate[z]
                if m not in partner:
                    break
                z = partner[m]
        chains.append(order)
        done |= {c for c, _ in order}
    status = np.concatenate([st_cut, st_join])
    if np.any(status != EDIT_OK):
        return None, status
    o = {k: np.array(s[k], dtype=np.int32, copy=True) for k in FIELDS}
    lens = s["len_bp"]

    def write(frags, label):
        tot = int(sum(int(lens[f]) for f, _ in frags))
        run = 0
        for p, (f, ori) in enumerate(frags):
            o["pos"][f] = p; o["id_c"][f] = label; o["start_bp"][f] = run; o["ori"][f] = ori; o["circ"][f] = 0
            o["prev"][f] = frags[p - 1][0] if p > 0 else -1
            o["next"][f] = frags[p + 1][0] if p + 1 < len(frags) else -1
            o["l_cont"][f] = len(frags); o["l_cont_bp"][f] = tot
            run += int(lens[f])

    in_chain = set()
    for order in chains:
        frags = []
        for c, z in order:
            p = pieces[c][0]
            frags += [(f, -ori) for f, ori in reversed(p)] if z & 1 else list(p)
            in_chain.add(c)
        write(frags, min(c for c, _ in order))
    for c, (p, ring, touched) in pieces.items():
        if c not in in_chain and touched:
            write(p, c)
    return o, status
