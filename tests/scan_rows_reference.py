"""A numpy restatement of the indexed contact producer (k_scan_rows): which ids a step affects, which slice of the sorted contact list
each of them owns, which contacts the pass must queue -- and the facts about a step's SHAPE that decide which parts of the kernel run:
how many rows are listed, how many go to one wave, how many trips a row takes, how many bitmap words a thread lists.

Nothing of the engine is in here: np.isin over the layout's contig labels, np.searchsorted over the row array.  The GPU tests
(tests/test_scan_rows_midsize_gpu.py) compare the engine's counters with `count` and assert from `shape` that a case reaches the branch
it is named for; tests/test_scan_rows_reference_cpu.py pins this file against the older numpy count, against the host's row index, bound
and switch, and shows that each `flaw` below -- a mistake the kernel could make -- changes the count of the case built to catch it.

The constants restate graal_amd/csrc/scan_rows.h and k_scan_rows' launch; the CPU test checks the one the library exports."""
import numpy as np

ROWS_CAP = 2048          # affected rows a step of the indexed pass may have (the kernel's LDS list)
ROWS_PER_TRIP = 512      # contacts of a row a wave takes per trip: 64 lanes x 8 col words
ROWS_THREADS = 256       # threads of a block: four waves
MAX_BLOCKS = 64
SWITCH_R = 16            # the shipped ratio of the switch

FLAWS = ("short_slice", "first_trip_only", "first_row_per_wave_only", "one_word_per_thread", "drop_listed_from")


def affected_ids(bin_of_sub, id_c, fA, fBs):
    """The ids of the contact list (sub-fragments) that belong to the contigs of fA and of the neighbours, in id order."""
    contigs = np.unique(np.asarray(id_c)[np.asarray([int(fA)] + [int(f) for f in fBs])])
    return np.flatnonzero(np.isin(id_c, contigs)[np.asarray(bin_of_sub)])


def shape_facts(n_rows, lengths, K, longest_contig, single_sub, n_ids):
    """What the host and the kernel make of a step with n_rows affected rows of the given lengths."""
    bound = (K + 1) * max(int(longest_contig), 1) * (1 if single_sub else 3)
    grid = max(1, min((bound + 3) // 4, MAX_BLOCKS))
    n_waves = grid * (ROWS_THREADS // 64)
    words = (int(n_ids) + 31) // 32 + 2
    lengths = np.asarray(lengths, np.int64)
    return dict(n_rows=int(n_rows), bound=int(bound), grid=int(grid), n_waves=int(n_waves),
                trips_per_wave=int(-(-int(n_rows) // n_waves)),             # rows the busiest wave (wave 0 of block 0) takes
                rows_over_512=int(np.count_nonzero(lengths > ROWS_PER_TRIP)),
                rows_over_1024=int(np.count_nonzero(lengths > 2 * ROWS_PER_TRIP)),
                longest_row=int(lengths.max()) if len(lengths) else 0,
                bitmap_words=int(words), words_per_thread=int(-(-words // ROWS_THREADS)))


def indexed_pass(row, col, bin_of_sub, id_c, fA, fBs, longest_contig, flaw=None, flaw_arg=None):
    """The indexed pass over a (row, col)-sorted list.  Returns a dict:

    ids     the affected ids, in id order (the kernel's row list);
    lo, hi  for each of them its slice [lo, hi) of the list;
    queued  the indices of the contacts the pass must queue (row AND col affected), ascending;
    per_row how many of them each listed row contributes;
    count   len(queued);
    shape   shape_facts of the step.

    `flaw` restates one mistake the kernel could make (FLAWS); the CPU test shows that each changes `count` where a case is built for it.
    """
    assert flaw is None or flaw in FLAWS
    row, col = np.asarray(row), np.asarray(col)
    assert np.all(row[1:] >= row[:-1]), "the indexed pass is defined for a list sorted by row"
    n_ids = len(bin_of_sub)
    single_sub = n_ids == len(id_c)
    ids = affected_ids(bin_of_sub, id_c, fA, fBs)
    mark = np.zeros(n_ids, bool)
    mark[ids] = True
    lo = np.searchsorted(row, ids, side="left").astype(np.int64)
    hi = np.searchsorted(row, ids + 1, side="left").astype(np.int64)
    shape = shape_facts(len(ids), hi - lo, len(fBs), longest_contig, single_sub, n_ids)
    listed = np.ones(len(ids), bool)
    if flaw == "first_row_per_wave_only":      # `i += n_waves` never loops
        listed[shape["n_waves"]:] = False
    elif flaw == "one_word_per_thread":        # the listing reads bitmap word t only
        listed[ids >= 32 * ROWS_THREADS] = False
    elif flaw == "drop_listed_from":           # the block-wide prefix loses the entries from position flaw_arg on
        listed[int(flaw_arg):] = False
    queued, per_row = [], np.zeros(len(ids), np.int64)
    for i in np.flatnonzero(listed):
        a, b = int(lo[i]), int(hi[i])
        if flaw == "short_slice":
            b = max(a, b - 1)
        elif flaw == "first_trip_only":        # the c0 loop never takes a second trip
            b = min(b, a + ROWS_PER_TRIP)
        hit = a + np.flatnonzero(mark[col[a:b]])
        per_row[i] = len(hit)
        queued.append(hit)
    queued = np.concatenate(queued) if queued else np.zeros(0, np.int64)
    return dict(ids=ids, lo=lo, hi=hi, queued=queued, per_row=per_row, count=int(len(queued)), shape=shape)


def switch_takes_index(shape, longest_row_of_list, nnz, R=SWITCH_R):
    """The engine's own choice for a step of this shape: rows fit the list and bound x longest row x R <= nnz."""
    return shape["bound"] <= ROWS_CAP and shape["bound"] * max(int(longest_row_of_list), 1) * R <= int(nnz)


def split_rows(row, index_sets):
    """For shards of one sorted list (index arrays, e.g. graal_amd.dist.shard_take per rank): the rows that have contacts in more than one
    shard, and per shard the rows of the whole list it holds nothing of."""
    row = np.asarray(row)
    all_rows = np.unique(row)
    held = [np.unique(row[ix]) for ix in index_sets]
    n_holders = np.zeros(int(row.max()) + 1 if len(row) else 1, np.int64)
    for h in held:
        n_holders[h] += 1
    return np.flatnonzero(n_holders > 1), [np.setdiff1d(all_rows, h) for h in held]
