// The shape of a candidate evaluation, decided in one place: which producer finds the step's contacts and with what grid, what the table
// kernel does itself, which finishing kernel goes out with the step or after the table kernel handed it back, and the grids, tiles and list
// sizes of those kernels; the full evaluation's kernels and grids too.  Pure arithmetic on a dozen facts about the problem, the call and a
// few adaptive flags (StepFacts): no HIP calls, no handle, no side effects -- the launchers of graal_hip.hip fill arguments and launch what
// a plan names, and every change of state stays with them.  Shared with host_check.cpp, so that the CPU tests pin every branch without a
// device (tests/test_step_plan_cpu.py).  What the rounds measured behind each choice: DESIGN_HISTORY.md, "The shape of a step".
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "strict_sets.h"
#include "scan_rows.h"

// what the kernels fix (graal_hip.hip asserts that they agree with its own constants)
constexpr int PLAN_MAXK = graal::US_MAXK;          // neighbours of a step at most
constexpr int PLAN_N_DONE = 16;                    // completion counters of the producers
constexpr int PLAN_STRICT_INLINE_M = 20;           // affected sets up to this many fragments are priced by the table block
constexpr int PLAN_SCAN_LDS_MAX = 48 * 1024;       // affected bitmap of the producers: 1 bit per contact-list id up to 393,216 ids, folded beyond

// the environment switches that shape a launch (graal_hip.hip: Env, read once per process), at their values when unset
struct PlanEnv {
    int scan_threads = 0, scan_groups = 4, scan_blocks = 256 * 2 - 16, scan_fold_bits = 0;
    long long scan_rows_r = 16;
    int fin_blocks = 0;
    bool strict_dense = false, no_flat = false, full_no_compact = false, full_no_lds = false;
    int full_mass_tiled = -1, stage_tables = -1;
};

// registers and LDS of k_tm and k_fin as the runtime reports them (queried once per process), and k_fin's dynamic LDS per neighbour
struct KernelFigures {
    size_t lds_tm = 64 * 1024, lds_fin = 32 * 1024;
    int regs_tm = 128, regs_fin = 128;
    size_t fin_dyn_lds_per_k = 0;
};

struct StepFacts {
    // the problem
    int n = 0, n_sub_total = 0;
    long long nnz = 0;
    bool single_sub = true;
    int n_contigs = 0, max_lcont = 0, lcont_bound = 0;   // (max_lcont: as last seen, one commit stale; lcont_bound: what it can be NOW)
    bool has_rep = false, has_ubins = false;             // repeated bins; bins whose sub-fragments carry different RF counts
    int uniform_accu = 0;
    bool strict = false, quirk = false;                  // GRAAL_MODE_STRICT, GRAAL_MODE_REF_TRANS_ACCU
    // the call
    int K = 1, world = 1;
    bool exchange = false, publish = false, ev = false;  // a host exchange is attached; the step publishes to the host; it carries an event pair
    // adaptive flags
    bool finisher_ok = true, spin_ok = true, gwait_env = true, mid_run = false;
    // the row index
    bool has_rowptr = false;
    long long longest_row = 0;
    int forced_producer = 0;                             // 1 streaming, 2 indexed (a switch, or a repeated step keeping its own), 0: decide
    // the unit list of the tiled reference-arithmetic kernels
    unsigned long long slist_soft_cap = 1ull << 23, slist_floor = 0, slist_cap = 0;
    PlanEnv env;
    KernelFigures kf;
};

// what everything that must HOLD a step is sized by: the bound of the longest contig
inline int plan_lc(const StepFacts& f) { return std::max(std::max(f.max_lcont, f.lcont_bound), 1); }

// ---- the producer (k_scan: one pass over the list; k_scan_rows: the affected rows through the row index)
// why_not: the indexed pass was forced and is impossible (static text), the step must fail; threads, groups: of the streaming pass (the
// indexed pass has its own fixed block); grid: of the producer chosen; bitmap_bytes: dynamic LDS of either; wmask all ones: every id has its
// own bit; done_inc: what the grid adds to each completion counter -- k_tm's finishing block waits for exactly these
struct ProducerPlan {
    bool indexed = false;
    const char* why_not = nullptr;
    int threads = 0, groups = 0, grid = 0, done_inc[PLAN_N_DONE] = {};
    size_t bitmap_bytes = 0;
    unsigned wmask = 0xffffffffu;
};

// one bit per contact-list id while they fit the LDS budget; beyond that the ids are folded onto 2^18 bits (false positives are dropped by
// the consumers' membership test, results unchanged).  GRAAL_SCAN_FOLD_BITS = b folds onto 2^b bits whatever the size
inline void plan_bitmap(const StepFacts& f, size_t* shm_out, unsigned* wmask_out)
{
    const int fold_bits = f.env.scan_fold_bits;
    size_t shm = (size_t)((f.n_sub_total + 31) / 32 + 2) * 4;
    unsigned wmask = 0xffffffffu;
    if (shm > (size_t)PLAN_SCAN_LDS_MAX || fold_bits) {
        const int b = fold_bits ? fold_bits : 18;
        if ((size_t)1 << b < (size_t)f.n_sub_total) { wmask = (1u << (b - 5)) - 1u; shm = ((size_t)1 << (b - 5)) * 4; }
    }
    *shm_out = shm; *wmask_out = wmask;
}

// bound on the rows a step can affect: K + 1 contigs of at most the longest contig's fragments, every sub-fragment of a bin a row of its own
inline long long plan_rows_bound(const StepFacts& f) { return scan_rows_bound(f.K, plan_lc(f), f.single_sub); }

// why the map has no indexed pass at all (null: it has one), and why this step cannot take it
inline const char* plan_no_index(const StepFacts& f, unsigned wmask)
{
    if (!f.has_rowptr) return "the contact list has no row index (it was not uploaded sorted by row)";
    if (wmask != 0xffffffffu) return "the affected bitmap is folded (more ids than LDS bits): no indexed pass";
    return nullptr;
}
inline const char* plan_rows_impossible(const StepFacts& f, unsigned wmask)
{
    if (const char* why = plan_no_index(f, wmask)) return why;
    if (plan_rows_bound(f) > (long long)ROWS_CAP) return "the contigs are too long for the indexed pass (more affected rows than its list holds)";
    return nullptr;
}

// Indexed iff possible and the contacts the pass can visit at worst, rows bound x longest row, are at most nnz / R (scan_rows.h; R = 16,
// GRAAL_SCAN_ROWS_R: reasoned in DESIGN.md section 4).  A step that carries an event pair streams: the pairs are pairs around the streaming
// kernel.  Per step, stateless; ranks may choose for themselves.
inline ProducerPlan plan_producer(const StepFacts& f)
{
    ProducerPlan p;
    plan_bitmap(f, &p.bitmap_bytes, &p.wmask);
    const char* why = plan_rows_impossible(f, p.wmask);
    if (f.forced_producer == 2 && why) p.why_not = why;
    p.indexed = f.forced_producer == 2 ? !why
                                       : (f.forced_producer == 0 && !f.ev && !why && scan_rows_wins(plan_rows_bound(f), f.longest_row, f.nnz, f.env.scan_rows_r));
    // streaming: 1024 threads (two blocks per CU) for the lists it is built for, 256 for a list that would fill only a handful of such blocks;
    // two 1024-thread blocks per CU fill the 256 CUs, 16 fewer leave room for k_tm's blocks, which run at the same time
    p.threads = f.env.scan_threads > 0 ? f.env.scan_threads : (f.nnz < 2000000 ? 256 : 1024);
    p.groups = f.env.scan_groups;
    if (p.indexed) {
        // a wave per row of the bound, four waves per block, a few dozen blocks at most (every block pays the prologue and the listing of the bitmap)
        p.grid = (int)std::max<long long>(1, std::min<long long>((plan_rows_bound(f) + 3) / 4, 64));
    } else {
        const long long groups = (f.nnz >> 2) + 1;
        const long long per_block = (long long)p.groups * p.threads;   // groups one block takes per iteration
        p.grid = (int)std::max<long long>(1, std::min<long long>((groups + per_block - 1) / per_block, f.env.scan_blocks));
    }
    for (int c = 0; c < PLAN_N_DONE; c++) p.done_inc[c] = (p.grid - c + PLAN_N_DONE - 1) / PLAN_N_DONE;
    return p;
}

// ---- the flow: what the table kernel does itself and what goes out with the step
enum Finisher { FIN_NONE, FIN_KFIN, FIN_FLAT, FIN_TILED };   // k_tm's last block / k_fin / k_strict_flat / k_gprep + k_strict2 (or the dense validation kernel)

// may this evaluation use k_strict_flat?  With several ranks (an exchange attached) too: every rank picks the same kernel, because the choice
// is the sets' geometry, the same on every rank
inline bool plan_flat_allowed(const StepFacts& f)
{
    return !f.env.no_flat && f.strict && !f.env.strict_dense && (f.world == 1 || f.exchange) && f.publish;
}

// The one rule for who finishes what k_tm does not: k_fin; in reference arithmetic the tiled kernels -- behind ONE try of k_strict_flat where
// the caller lets it go first (small sets; if they are not, it hands the step back again)
inline Finisher plan_finisher(const StepFacts& f, bool flat_first)
{
    return !f.strict ? FIN_KFIN : ((flat_first && plan_flat_allowed(f)) ? FIN_FLAT : FIN_TILED);
}

// late_stage: a few long contigs hold nearly every fragment, the finisher goes out right behind the scan; mid: k_strict_flat goes out behind
// every scan and k_tm prices nothing itself (one rank only); tm_publishes: k_tm's last block finishes the step when the work is small, and
// says so if not; rep_delta: k_rep_delta goes out (the repeated bins' pixels, densely); fin_wait_ticks: how long a kernel waits for the scan
struct FlowPlan {
    bool late_stage = false, mid = false, tm_publishes = false, rep_delta = false;
    int strict_inline_m = 0, stage_tables = 0, fin_wait_ticks = 0;
    Finisher finisher = FIN_NONE;
};

inline FlowPlan plan_flow(const StepFacts& f, bool indexed)
{
    FlowPlan p;
    p.late_stage = f.max_lcont > 128 && (long long)f.n_contigs * 64 < (long long)f.n;
    p.mid = plan_flat_allowed(f) && f.world == 1 && f.mid_run && !p.late_stage && f.finisher_ok;
    p.strict_inline_m = f.env.strict_dense ? -1 : (p.mid ? 0 : PLAN_STRICT_INLINE_M);
    // k_tm copies its tables under a long scan only; the indexed pass is always a short one (GRAAL_STAGE_TABLES = 0 / 1 overrides)
    p.stage_tables = f.env.stage_tables >= 0 ? (f.env.stage_tables ? 1 : 0) : ((!indexed && f.nnz >= 4000000) ? 1 : 0);
    p.tm_publishes = f.publish && (f.world == 1 || f.exchange) && f.finisher_ok && !f.has_rep && !p.late_stage && !p.mid && !(f.strict && f.env.strict_dense);
    // a generous multiple of the time the streaming pass needs at 2 TB/s, plus launch slack (100 MHz ticks)
    p.fin_wait_ticks = (int)std::min<long long>(100ll * 50 + (long long)(4.0 * 4.0 * (double)f.nnz / 2.0e12 * 1.0e8), 1ll << 30);
    p.rep_delta = f.has_rep;
    // (several ranks: whoever finishes a step that is not in the late stage goes through k_strict_flat first, like a rank that k_tm sent there)
    p.finisher = p.tm_publishes ? FIN_NONE : plan_finisher(f, p.mid || (f.world > 1 && !p.late_stage));
    return p;
}

// ---- k_fin
struct FinPlan { int grid = 0; bool event = false; };   // event: the grid could keep k_tm off the chip while it spins for k_tm's tables: ordered behind k_tm instead

// the largest grid of k_fin that leaves room for a block of k_tm on every CU, in registers AND in LDS
inline int plan_fin_no_wait(const StepFacts& f)
{
    const size_t lds_cu = 160 * 1024;   // gfx950
    const int regs_simd = 512;          // VGPRs per lane and SIMD; a 256-thread block puts one wave on each SIMD
    const auto up8 = [](int r) { return (r + 7) & ~7; };
    const int by_lds = (int)((lds_cu - std::min(lds_cu, f.kf.lds_tm)) / (f.kf.lds_fin + (size_t)f.K * f.kf.fin_dyn_lds_per_k));
    const int by_regs = (regs_simd - up8(f.kf.regs_tm)) / up8(f.kf.regs_fin);
    return 256 * std::max(1, std::min(by_lds, by_regs));
}

// short contigs leave k_fin a handful of contacts: a small grid; contigs of a few hundred fragments: the largest grid that may spin for
// k_tm's tables; contigs of thousands: the whole chip four times over, behind an event
inline FinPlan plan_fin(const StepFacts& f)
{
    FinPlan p;
    const int no_wait = plan_fin_no_wait(f);
    if (f.env.fin_blocks > 0) p.grid = f.env.fin_blocks;
    else if (f.max_lcont > 0 && f.max_lcont <= 16) p.grid = 32;
    else p.grid = f.max_lcont > 1024 ? 2048 : std::min(768, no_wait);
    p.event = p.grid > no_wait;
    return p;
}

// ---- reference arithmetic, the tiled kernels (k_gprep + k_strict2)
// dense: GRAAL_STRICT_DENSE, the O(m^2) validation kernel instead -- nothing else applies; nt: bound on the tiles of the union set, refused
// at 65,536 or more (the step fails); seg_unit: fragments of the segment side per entry of the unit list; target: units the grid wants before
// k_strict2 merges neighbouring entries; worst: the list with EVERY tile pair of the largest union listed; need: entries this step's list must
// hold; alloc: entries to allocate (0: the list is long enough); gwait: k_strict2 follows k_gprep through its word in memory, not an event
struct StrictPlan {
    bool dense = false, refused = false, gwait = false;
    int grid = 0, tile = 0, seg_unit = 0, cull_blocks = 0, no_window = 0;
    unsigned long long nt = 0, target = 0, worst = 0, need = 0, alloc = 0;
};

inline StrictPlan plan_strict(const StepFacts& f)
{
    StrictPlan p;
    p.dense = f.env.strict_dense;
    if (p.dense) return p;
    const int lc = plan_lc(f);
    // the GRID by the longest contig as last seen (a performance choice); everything that must hold the step by the bound
    const int lg = std::max(f.max_lcont, 1);
    p.grid = lg <= 64 ? 32 : (lg <= 256 ? 512 : 1024);
    // fragments per tile: 64 (one per lane); with several sub-fragments per bin 32 (the halves of a wave hold the same 32 fragments)
    p.tile = f.single_sub ? 64 : 32;
    // at most K + 1 contigs, at most every fragment; + one partial tile per global piece
    p.nt = std::min<unsigned long long>((unsigned long long)(f.K + 1) * (unsigned long long)((lc + p.tile - 1) / p.tile),
                                        (unsigned long long)((f.n + p.tile - 1) / p.tile + f.K + 1)) + (unsigned long long)graal::US_MAXP;
    p.refused = p.nt >= 65536ull;
    // longer entries once a contig may exceed 512 bins
    p.seg_unit = f.single_sub ? (lc > 512 ? 16 : 4) : (lc > 512 ? 4 : 2);
    p.target = 24ull * (unsigned long long)p.grid;   // 6 per wave
    // sized once per layout size, for the largest union n fragments and MAXK neighbours can form.  One rank: the soft cap to begin with, raised
    // when a step's list overflowed; several ranks: the worst case (a repeated step on ONE rank would leave the ranks out of step)
    const unsigned long long nt_n = (unsigned long long)((f.n + p.tile - 1) / p.tile + PLAN_MAXK + 1) + (unsigned long long)graal::US_MAXP;
    p.worst = (nt_n * (nt_n + 1ull) / 2ull) * (unsigned long long)(p.tile / p.seg_unit) + 64ull;
    p.need = (f.world == 1 && f.publish) ? std::min(p.worst, std::max(f.slist_soft_cap, f.slist_floor)) : p.worst;
    p.alloc = p.need > f.slist_cap ? std::max<unsigned long long>(p.need, 64ull) : 0ull;
    // only a grid that leaves room for k_gprep's blocks on every CU may wait for them in the kernel, only one rank, only while the engine's
    // streams are known to run side by side
    p.gwait = f.gwait_env && f.publish && f.world == 1 && f.spin_ok && p.grid <= 512;
    p.cull_blocks = (int)std::min<unsigned long long>(1024ull, std::max<unsigned long long>(1ull, p.nt));
    p.no_window = (f.quirk && f.has_ubins) ? 1 : 0;
    return p;
}

// ---- the full evaluation
enum FullNnz { FULL_NNZ_NONE, FULL_NNZ_PLAIN, FULL_NNZ_U, FULL_NNZ_L };   // no contacts / k_full_nnz / k_full_nnz_u / k_full_nnz_l
enum FullMass { FULL_MASS_64, FULL_MASS_16, FULL_MASS_T };                // k_full_mass<64> / <16> / k_full_mass_t

// compact: every sub-fragment has the same RF count, the compact records; lab_bytes: k_full_nnz_l's labels in LDS; S: waves that share an
// x tile (k_full_mass_t)
struct FullPlan {
    bool compact = false;
    FullNnz nnz_kernel = FULL_NNZ_NONE;
    FullMass mass_kernel = FULL_MASS_64;
    int nnz_grid = 0, mass_grid = 0, S = 0;
    size_t lab_bytes = 0;
};

constexpr int PLAN_FULL_G = 2;   // groups of 4 contacts every lane of the contacts' kernels takes per iteration

inline FullPlan plan_full(const StepFacts& f)
{
    constexpr int FG = PLAN_FULL_G;
    FullPlan p;
    p.compact = f.uniform_accu > 0 && !f.env.full_no_compact;
    if (f.nnz) {
        const long long groups = (f.nnz >> 2) + 1;
        // labels in LDS: uniform RF counts, a list worth it, and 2 bytes per sub-fragment within 150 KB of LDS
        p.lab_bytes = 2 * (((size_t)f.n_sub_total + 7) & ~(size_t)7);
        if (p.compact && !f.env.full_no_lds && f.nnz >= 2000000 && p.lab_bytes <= 150 * 1024) {
            p.nnz_kernel = FULL_NNZ_L;
            p.nnz_grid = (int)std::max<long long>(1, std::min<long long>((groups + 1024 * FG - 1) / (1024 * FG), 256));
        } else {
            p.nnz_kernel = p.compact ? FULL_NNZ_U : FULL_NNZ_PLAIN;
            p.nnz_grid = (int)std::max<long long>(1, std::min<long long>((groups + 256 * FG - 1) / (256 * FG), 256 * 8));   // 8 blocks of 256 threads per CU
        }
    }
    const int lc = plan_lc(f);
    // long contigs in a large map: the tiled kernel, S waves sharing an x tile so that the grid has a few thousand waves whatever the contigs'
    // length; maps of a few thousand bins keep the kernel with one WAVE per fragment
    if (f.env.full_mass_tiled == 1 || (f.env.full_mass_tiled != 0 && lc > 256 && f.n > 16384)) {
        p.mass_kernel = FULL_MASS_T;
        p.S = std::min(16, std::max(1, ((std::min(lc, f.n) + 63) / 64 + 7) / 8));
        p.mass_grid = (((f.n + 63) / 64) * p.S + 3) / 4;
    } else if (f.n <= 16384) {
        p.mass_kernel = FULL_MASS_64;
        p.mass_grid = (f.n + 3) / 4;
    } else {
        p.mass_kernel = FULL_MASS_16;
        p.mass_grid = (f.n + 15) / 16;
    }
    return p;
}
