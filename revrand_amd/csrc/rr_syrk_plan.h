// Host-side planner of the Gram launchers (rr_launch_syrk_f32 / _f64 in rr_rff.hip, rr_launch_syrk_bf16 in rr_syrk16.hip):
// which kernels a Gram takes, in which tile order and with which K-splits, as a function of the padded shape, the CU
// count and the environment switches -- no HIP, no context: the launchers execute a plan, rr_syrk_plan (the C ABI) and
// tests/syrk_plan_sweep.cpp read one without a GPU.  Also the tile constants the plans need and the XCD tile map.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <vector>

// columns per tile side and rows per k-block: the f32 / split 16-bit tiles (those engines' k-step pairs: 64 rows), the small f32
// kernel's and the f64 ones; XCDs the tile map deals the tiles to
constexpr int GR_TC = 256, GR_KB = 32, GS_TC = 128, GS_KB = 32, G64_TC = 128, G64_KB = 16, SYRK_NXCD = 8;

// Every environment switch the three launchers read, parsed in one place (measurements: docs/KERNELS.md 8.1).  Two
// conventions, as ever: "set" = the variable exists, whatever its value; "= v" = it exists and atoi gives v.
struct SyrkSwitches {
    int64_t rows_per_split = 0;
    int ablate = 0, stagger = 3;
    bool no_tile_map = false, no_diag_kernel = false, no_ragged_kernel = false, ablate_set = false, diag_kb64_now = false,
         no_diag16_now = false, small_off = false, no_split_search = false, w8 = false, merge_diag = false, no_diag16 = false,
         diag_kb64 = false, fine64_off = false, tri64_off = false;
};

inline SyrkSwitches rr_syrk_switches() {
    auto is = [](const char *name, int v) { const char *e = getenv(name); return e != nullptr && atoi(e) == v; };
    auto nonzero = [](const char *name) { const char *e = getenv(name); return e != nullptr && atoi(e) != 0; };
    static const SyrkSwitches once = [&] {  // ---- read once per process
        SyrkSwitches s;
        s.small_off = is("RR_SYRK_SMALL", 0);                 // never the 128 x 128 small kernel
        s.no_split_search = is("RR_SYRK_SPLIT_SEARCH", 0);    // small inputs keep small_split's count
        s.stagger = getenv("RR_SYRK_STAGGER") ? atoi(getenv("RR_SYRK_STAGGER")) : 3;  // 0 / 1 / 2: the flat / flat staggered / buffer-descriptor main kernel
        s.w8 = nonzero("RR_SYRK_W8");                         // the 8-wave main kernel
        s.merge_diag = nonzero("RR_SYRK_MERGE_DIAG");         // off-diagonal and diagonal tiles in one launch
        s.no_diag16 = getenv("RR_SYRK_NO_DIAG16") != nullptr; // set: the whole-block diagonal kernel
        s.diag_kb64 = is("RR_SYRK_DIAG_KB", 64);              // rr_syrk_f32_diag16_kernel<64> where the splits allow
        s.fine64_off = is("RR_SYRK64_FINE_SPLIT", 0);         // no 128-row splits for the posterior's square operand
        s.tri64_off = is("RR_SYRK64_TRI", 0);                 // the f64 kernels ignore lower_tri
        return s;
    }();
    SyrkSwitches s = once;                                    // ---- read on every call
    const char *renv = getenv("RR_GRAM_ROWS_PER_SPLIT"), *aenv = getenv("RR_GRAM_ABLATE");
    s.rows_per_split = renv ? atoll(renv) : 0;                // every kernel's rows per K-split (rounded down to its k-block)
    s.no_tile_map = getenv("RR_GRAM_NO_TILE_MAP") != nullptr;            // set: plain tile order
    s.no_diag_kernel = getenv("RR_SYRK_NO_DIAG_KERNEL") != nullptr;      // set: the diagonal tiles stay in the main kernel (f32, f64)
    s.no_ragged_kernel = getenv("RR_SYRK_NO_RAGGED_KERNEL") != nullptr;  // set: a ragged last block stays in the main kernel
    s.ablate_set = aenv != nullptr;                           // RR_GRAM_ABLATE set: never the small kernel, and ...
    s.ablate = aenv ? atoi(aenv) : 0;                         // ... its value: SyrkArgs::ablate, non-zero takes the flat main kernel
    s.diag_kb64_now = is("RR_SYRK_DIAG_KB", 64);              // at this call: the diagonal kernel's rows per split in 64s
    s.no_diag16_now = getenv("RR_SYRK_NO_DIAG16") != nullptr; // at this call: no merged launch
    return s;
}

enum SyrkKernel {
    SK_NONE = 0, SK_F32_SMALL, SK_F32_MAIN, SK_F32_W8, SK_F32_FLAT, SK_F32_FLATSTAG, SK_F32_BUF, SK_F32_RAGGED, SK_F32_DIAG,
    SK_F32_DIAG16_32, SK_F32_DIAG16_64, SK_F32_MERGED, SK_F64, SK_F64_DIAG, SK_B16W4
};
enum SyrkRoute { SR_SMALL = 0, SR_MAIN, SR_MERGED, SR_F64, SR_SPLIT16 };
// one kernel of a route (SK_NONE: not launched): workgroups = nsplit x its tiles, rows per K-split, K-splits
struct SyrkLaunch { int kernel = SK_NONE; int64_t grid = 0, rps = 0, nsplit = 0; };

struct SyrkPlan {
    int err = 0;             // 0, or the status (RR_ERR_INVALID = -1) the launcher returns with msg
    char msg[256] = "";
    int route = SR_MAIN, nb_all = 0;  // nb_all: column blocks of the padded matrix
    int nb = 0, ntiles = 0;  // the off-diagonal (or only) kernel's blocks and tiles per K-split
    int od = 0, rg = 0;      // diagonal tiles / a ragged last block in kernels of their own
    bool use_map = false;    // the XCD tile map of (nb, od)
    int ablate = 0, lower_tri = 0;
    int64_t rows = 0, slabs = 0;   // rows the kernels walk (split engines: padded to 64); deterministic mode: slabs = K-splits to reduce
    SyrkLaunch off, ragged, diag;  // off: off-diagonal / small / split-engine kernel; SR_MERGED: off + diag are ONE launch
};

template <typename... A> inline SyrkPlan &rr_plan_fail(SyrkPlan &p, const char *fmt, A... a) {
    p.err = -1;
    snprintf(p.msg, sizeof p.msg, fmt, a...);
    return p;
}
inline int64_t rr_gcd64(int64_t x, int64_t y) { return y ? rr_gcd64(y, x % y) : x; }

// `wg` equal-cost workgroups per K-split on `slots` places: the split count in [ns_first, ns_last] whose workgroups fill
// whole rounds best while a split keeps min_rows rows (the first of equals; `fallback` if not even ns_first does)
inline int64_t best_fill_splits(int64_t ns_first, int64_t ns_last, int64_t wg, int64_t slots, int64_t rows, int64_t min_rows,
                                int64_t fallback) {
    double best = -1.0;
    for (int64_t ns = ns_first; ns <= ns_last; ++ns) {
        if (rows / ns < min_rows && ns > 1) break;
        const int64_t rounds = (ns * wg + slots - 1) / slots;
        const double eff = (double)(ns * wg) / (double)(rounds * slots);
        if (eff > best + 1e-9) best = eff, fallback = ns;
    }
    return fallback;
}

// G(upper) += P^T P of a zero-padded f32 feature matrix (rows % 32 == 0, ldp % 256 == 0).  engine: the context's
// gram_engine -- non-zero hands the call to the split 16-bit launcher (route SR_SPLIT16, nothing else filled in).
inline SyrkPlan rr_plan_syrk_f32(int64_t rows, int64_t ldp, int F, int rider, int num_cu, int deterministic,
                                 const SyrkSwitches &sw, int engine = 0) {
    SyrkPlan p;
    p.rows = rows;
    if (engine != 0) {
        p.route = SR_SPLIT16;
        if (rider) return rr_plan_fail(p, "%s", "gram: the rider column needs the f32 engine");
        return deterministic ? rr_plan_fail(p, "%s", "gram: deterministic mode (rr_set_deterministic) needs the f32 engine, not a split 16-bit one") : p;
    }
    if (rider && !(F < ldp)) return rr_plan_fail(p, "%s", "gram: no pad column for the rider");
    const int nb_all = p.nb_all = (int)(ldp / GR_TC);
    // small feature counts over few rows: 128 x 128 tiles (rr_syrk_f32_small_kernel)
    // (where it wins, tools/small_gram_bench.py: while the 256 x 256 tiles x 1024-row splits cannot give every CU a workgroup --
    // F = 512: up to ~85 000 rows (10 000 rows: 0.148 against 0.200 ms per pass), F = 1024: up to ~26 000; above that the big
    // tiles' LDS-DMA pipeline is 2-3x faster per flop than this kernel's register-staged loads)
    const int64_t big_tiles = (ldp / GR_TC) * (ldp / GR_TC + 1) / 2;
    if (!sw.small_off && ldp <= 1024 && big_tiles * ((rows + 1023) / 1024) < num_cu && rows % GS_KB == 0 && !sw.ablate_set) {
        p.route = SR_SMALL, p.nb = (int)(ldp / GS_TC), p.ntiles = p.nb * (p.nb + 1) / 2;
        // K-splits: enough workgroups for every CU (two fit one), at least 128 rows and at most 32768 each
        int64_t ns = std::max<int64_t>((2 * num_cu + p.ntiles - 1) / p.ntiles, (rows + 32767) / 32768);
        ns = std::min<int64_t>(ns, std::max<int64_t>(rows / 128, 1));
        const int64_t rps = ((rows + ns - 1) / ns + GS_KB - 1) / GS_KB * GS_KB;
        ns = (rows + rps - 1) / rps;
        p.off = {SK_F32_SMALL, ns * p.ntiles, rps, ns};
        p.slabs = deterministic ? ns : 0;
        return p;
    }
    const int od = p.od = (nb_all >= 2 && !sw.no_diag_kernel) ? 1 : 0;  // diagonal tiles in their own kernel
    // ragged last block (<= 192 valid columns): its off-diagonal tiles go to rr_syrk_f32_ragged_kernel, and the main
    // kernel enumerates the tiles among the first nb_all - 1 blocks only
    const int w_last = F + (rider ? 1 : 0) - GR_TC * (nb_all - 1);
    const int rg = p.rg = (od && nb_all >= 3 && w_last <= 192 && !sw.no_ragged_kernel) ? 1 : 0;
    const int nb = p.nb = nb_all - rg;
    const int ntiles = p.ntiles = od ? nb * (nb - 1) / 2 : nb * (nb + 1) / 2;
    p.use_map = (ntiles % SYRK_NXCD == 0) && !sw.no_tile_map;
    // K-splits: f32 accumulation over <= 32768 rows per split.  Workgroups of one kernel all cost the same, so
    // each kernel gets the split count that makes ITS workgroup count (close to) a multiple of the CU count:
    // exactly for the off-diagonal kernel (nsplit = k * CUs / gcd(CUs, ntiles), k minimal), by search for the
    // diagonal one (nb workgroups per split; an odd nb would otherwise force CUs splits on both).
    const int64_t total_tiles = (int64_t)nb_all * (nb_all + 1) / 2;
    const int64_t min_splits = (rows + 32767) / 32768;
    auto rows_per = [&](int64_t ns) { return ((rows + ns - 1) / ns + GR_KB - 1) / GR_KB * GR_KB; };
    const int64_t unit = ntiles > 0 ? num_cu / rr_gcd64(num_cu, ntiles) : 1;
    int64_t nsplit = (min_splits + unit - 1) / unit * unit;
    // small inputs: just cover the rows, >= 1024 per split -- unless that leaves most CUs without a workgroup (few tiles:
    // config 1's F = 512 is ONE off-diagonal tile and two diagonal ones, 10 splits of its 10 000 rows = 10 workgroups of
    // 32 k-blocks at one CU's rate each): then down to 256 rows per split, until the tiles x splits fill the CUs
    // (config 1's `_elbo`: 1.42 -> 1.13 ms)
    auto floor_rows = [&](int64_t tiles_per_split) { return tiles_per_split * ((rows + 1023) / 1024) < num_cu ? (int64_t)256 : (int64_t)1024; };
    auto small_split = [&](int64_t tiles_per_split) {
        const int64_t fr = floor_rows(tiles_per_split);
        if (fr == 1024) return (rows + 1023) / 1024;
        const int64_t want = (num_cu + tiles_per_split - 1) / std::max<int64_t>(tiles_per_split, 1);
        return std::min((rows + fr - 1) / fr, std::max((rows + 1023) / 1024, want));
    };
    if (rows / nsplit < 1024) {
        nsplit = small_split(std::max(ntiles, 1));
        // (round 6) ... and among the split counts around it, the one whose workgroups finish soonest: time ~ rounds x (rows per
        // split + a workgroup's prologue and 64k-entry atomic epilogue, ~96 rows' worth).  F = 1024, N = 44 484 (the reference's
        // SARCOS shape): 44 splits x 6 tiles = 264 workgroups were TWO rounds on 256 CUs, the second with 8 workgroups.
        if (ntiles > 0 && !sw.no_split_search) {
            double best_cost = 1e300;
            int64_t best_ns = nsplit;
            const int64_t ns_hi = std::max<int64_t>(rows / 256, 1), ns_lo = std::max<int64_t>(rows / 32768, 1);
            for (int64_t ns = ns_lo; ns <= ns_hi && ns <= ns_lo + 4096; ++ns) {
                const int64_t rp = rows_per(ns), n2 = (rows + rp - 1) / rp;
                const int64_t rounds = ((int64_t)ntiles * n2 + num_cu - 1) / num_cu;
                const double cost = (double)rounds * ((double)rp + 96.0);
                if (cost < best_cost - 1e-9) best_cost = cost, best_ns = n2;
            }
            nsplit = best_ns;
        }
    }
    if (nsplit < 1) nsplit = 1;
    int64_t rps = rows_per(nsplit), rps_d = rps, rps_r = rps;
    if (od) {  // nb_all equal-cost workgroups per split
        rps_d = rows_per(best_fill_splits(min_splits, min_splits + 95, nb_all, num_cu, rows, floor_rows(nb_all), nsplit));
        if (rows % 64 == 0 && sw.diag_kb64_now) rps_d = (rps_d + 63) / 64 * 64;  // whole 64-row k-blocks for rr_syrk_f32_diag16_kernel<64>
    }
    if (rg)  // nb_all - 1 equal-cost workgroups per split
        rps_r = rows_per(best_fill_splits(min_splits, min_splits + 95, nb_all - 1, num_cu, rows, floor_rows(nb_all - 1), nsplit));
    if (sw.rows_per_split >= GR_KB) rps = rps_d = rps_r = (sw.rows_per_split / GR_KB) * GR_KB;
    if (deterministic) rps_d = rps_r = rps;  // one slab per K-split, shared by the three kernels
    nsplit = (rows + rps - 1) / rps;
    const int64_t nsplit_d = (rows + rps_d - 1) / rps_d, nsplit_r = (rows + rps_r - 1) / rps_r;
    if (!(nsplit * total_tiles < (int64_t)1 << 31 && nsplit_d * nb_all < (int64_t)1 << 31 && nsplit_r * nb_all < (int64_t)1 << 31))
        return rr_plan_fail(p, "%s", "gram: grid too large");
    p.ablate = sw.ablate;
    p.slabs = deterministic ? nsplit : 0;
    if (sw.merge_diag && od && !rg && ntiles > 0 && sw.stagger == 3 && !p.ablate && !sw.no_diag16_now) {
        p.route = SR_MERGED;
        p.off = {SK_F32_MERGED, nsplit * ntiles, rps, nsplit};
        p.diag = {SK_F32_MERGED, nsplit_d * nb_all, rps_d, nsplit_d};
        return p;
    }
    if (ntiles > 0) {
        const int k = (sw.stagger == 1 && !p.ablate) ? SK_F32_FLATSTAG : (sw.stagger == 2 && !p.ablate) ? SK_F32_BUF :
                      (sw.stagger == 0 || p.ablate) ? SK_F32_FLAT  // (the ablation switches live in the flat variant)
                      : sw.w8 ? SK_F32_W8 : SK_F32_MAIN;
        p.off = {k, nsplit * ntiles, rps, nsplit};
    }
    if (rg) p.ragged = {SK_F32_RAGGED, nsplit_r * (nb_all - 1), rps_r, nsplit_r};
    if (od)  // diagonal blocks as 16x16 sub-blocks; <64>: 64-row k-blocks when every K-split holds whole ones
        p.diag = {sw.no_diag16 ? SK_F32_DIAG : (sw.diag_kb64 && rows % 64 == 0 && rps_d % 64 == 0) ? SK_F32_DIAG16_64 : SK_F32_DIAG16_32,
                  nsplit_d * nb_all, rps_d, nsplit_d};
    return p;
}

// The same for a zero-padded f64 matrix (rows % 16 == 0, ldp % 128 == 0); lower_tri: P is square and lower triangular
inline SyrkPlan rr_plan_syrk_f64(int64_t rows, int64_t ldp, int F, int lower_tri, int num_cu, int deterministic,
                                 const SyrkSwitches &sw) {
    (void)F;
    SyrkPlan p;
    p.route = SR_F64;
    p.rows = rows;
    const int nb = p.nb = p.nb_all = (int)(ldp / G64_TC);
    const int od = p.od = (nb >= 2 && !sw.no_diag_kernel) ? 1 : 0;  // diagonal tiles in their own kernel
    const int ntiles = p.ntiles = od ? nb * (nb - 1) / 2 : nb * (nb + 1) / 2;
    const int64_t slots = (int64_t)num_cu * 2;  // two workgroups per CU
    // equal-cost workgroups: make their count a multiple of the slots (no partial last round) while a split keeps
    // >= 2048 rows; otherwise ~4 rounds
    const int64_t unit = slots / rr_gcd64(slots, ntiles);
    // (the posterior's C = Y^T Y at small F -- a square, triangular operand of <= 2048 rows: a few tiles whose k-loops are the
    // whole launch -- splits down to 128 rows: at F = 1024 two splits of 512 rows left 56 workgroups walking up to 32
    // k-blocks each, 69 + 40 us for a third of a GFLOP)
    const int64_t min_rows = (lower_tri && rows == ldp && rows <= 2048 && !sw.fine64_off) ? 128 : 512;
    int64_t nsplit = unit;
    if (rows / nsplit < 2048) nsplit = (slots * 4 + ntiles - 1) / ntiles;
    if (rows / nsplit < min_rows) nsplit = (rows + min_rows - 1) / min_rows;
    if (nsplit < 1) nsplit = 1;
    auto rows_per = [&](int64_t ns) { return ((rows + ns - 1) / ns + G64_KB - 1) / G64_KB * G64_KB; };
    const int64_t rps = rows_per(nsplit);
    nsplit = (rows + rps - 1) / rps;
    if (!(nsplit * ntiles < (int64_t)1 << 31)) return rr_plan_fail(p, "%s", "gram: grid too large");
    p.lower_tri = lower_tri && !sw.tri64_off && rows == ldp ? 1 : 0;
    p.slabs = deterministic ? nsplit : 0;
    if (ntiles > 0) p.off = {SK_F64, nsplit * ntiles, rps, nsplit};
    if (od) {
        // the diagonal kernel's own K-split: nb equal-cost workgroups per split, up to 4 resident per CU (36 KiB of LDS
        // each); the split count whose workgroup count fills whole rounds best while a split keeps >= min_rows rows
        const int64_t dslots = (int64_t)num_cu * 4;
        int64_t rps_d = rows_per(best_fill_splits(1, 4 * dslots / nb + 1, nb, dslots, rows, min_rows, 1));
        if (deterministic) rps_d = rps;  // one slab per K-split, shared by both kernels
        const int64_t nsd = (rows + rps_d - 1) / rps_d;
        p.diag = {SK_F64_DIAG, nsd * nb, rps_d, nsd};
    }
    return p;
}

// The split 16-bit engines (rr_syrk_b16w4_kernel): every upper tile in one kernel over rows padded to 64
inline SyrkPlan rr_plan_syrk_split16(int64_t rows, int64_t ldp, int F, int fp16, int num_cu, const SyrkSwitches &sw) {
    (void)F;
    SyrkPlan p;
    p.route = SR_SPLIT16;
    const int nb = p.nb = p.nb_all = (int)(ldp / GR_TC);
    const int ntiles = p.ntiles = nb * (nb + 1) / 2;
    p.use_map = (ntiles % SYRK_NXCD == 0) && !sw.no_tile_map;
    const int64_t rows64 = p.rows = (rows + 63) / 64 * 64;
    // f32 accumulation per K-split: the fp16 engine is accurate enough (max error = the f32 engine's) for the pipe's
    // accumulate bias to show in trace(G) -- 1.0e-6 of N at 32 768 rows per split, 6e-7 at 16 384 (+1.3 % time)
    const int64_t max_rows_split = fp16 ? 16384 : 32768;
    const int64_t min_splits = (rows64 + max_rows_split - 1) / max_rows_split;
    const int64_t unit = num_cu / rr_gcd64(num_cu, ntiles);
    int64_t nsplit = (min_splits + unit - 1) / unit * unit;
    if (rows64 / nsplit < 1024) nsplit = (rows64 + 1023) / 1024;
    if (nsplit < 1) nsplit = 1;
    int64_t rps = ((rows64 + nsplit - 1) / nsplit + 63) / 64 * 64;
    // the kernel's LDS-DMA addresses a K-split's stages through ONE buffer descriptor with 32-bit offsets: stage g of the
    // split sits g * ldp * 64 bytes behind its first (a wide matrix or a large RR_GRAM_ROWS_PER_SPLIT would wrap silently
    // and the Gram would be wrong): the launcher's own splits are halved until they fit, a forced one is refused
    auto wraps = [&](int64_t r) { return (r / 16) * ldp * 64 + 32768 >= (int64_t)1 << 31; };
    if (sw.rows_per_split >= 64) rps = (sw.rows_per_split / 64) * 64;
    else
        while (rps > 64 && wraps(rps)) rps = (rps / 2 + 63) / 64 * 64;
    nsplit = (rows64 + rps - 1) / rps;
    if (!(nsplit * ntiles < (int64_t)1 << 31)) return rr_plan_fail(p, "%s", "gram: grid too large");
    if (wraps(rps))
        return rr_plan_fail(p, "gram (split 16-bit engine): %lld rows per K-split of a %lld-column feature matrix exceed the kernel's "
                               "32-bit stage offsets: lower RR_GRAM_ROWS_PER_SPLIT", (long long)rps, (long long)ldp);
    p.ablate = sw.ablate;
    p.off = {SK_B16W4, nsplit * ntiles, rps, nsplit};
    return p;
}

// Greedy XCD-aware tile order: dispatch position q goes to XCD q % 8, so XCD x receives positions
// x, x+8, ...; fill each XCD's quota with tiles that add the fewest new column blocks to the set it
// already reads.  Only used when ntiles is a multiple of 8 (equal quotas keep the load balanced).
inline void rr_build_tile_map_uncached(int nb, int od, int nxcd, std::vector<int> &map) {
    const int ntiles = od ? nb * (nb - 1) / 2 : nb * (nb + 1) / 2;
    map.assign(ntiles, 0);
    std::vector<int> ta(ntiles), tb(ntiles);
    for (int a = 0, t = 0; a < nb; ++a)
        for (int b2 = a + od; b2 < nb; ++b2, ++t) { ta[t] = a; tb[t] = b2; }
    std::vector<char> used(ntiles, 0);
    const int quota = ntiles / nxcd;
    std::vector<int> part(ntiles, 0);  // tile -> XCD
    // greedy start: every XCD in turn takes the tiles that add the fewest new column blocks to what it already reads
    for (int x = 0; x < nxcd; ++x) {
        std::vector<char> have(nb, 0);
        for (int s = 0; s < quota; ++s) {
            int best = -1, bestcost = 1 << 30;
            for (int t = 0; t < ntiles; ++t) {
                if (used[t]) continue;
                const int cost = (have[ta[t]] ? 0 : 1) + ((have[tb[t]] || tb[t] == ta[t]) ? 0 : 1);
                if (cost < bestcost) { bestcost = cost; best = t; }
            }
            used[best] = 1;
            have[ta[best]] = have[tb[best]] = 1;
            part[best] = x;
        }
    }
    // ... improved by annealing over tile SWAPS between XCDs (round 5; RR_GRAM_TILE_ANNEAL=0: the greedy map).  The cost is
    // what the eight L2s read per row split: the number of distinct column blocks of P each XCD's tiles touch, summed --
    // 65 for the greedy partition of F = 4096's 120 off-diagonal tiles, 57 after annealing (a (16, 6, 1) design, 48, does not
    // exist); 141 -> 130 at 32 column blocks.  Deterministic (fixed seed); made once per process and tile count (cache below).
    static const bool anneal = !(getenv("RR_GRAM_TILE_ANNEAL") && atoi(getenv("RR_GRAM_TILE_ANNEAL")) == 0);
    if (anneal && nxcd > 1 && ntiles >= 2 * nxcd && nb <= 128) {
        std::vector<int> cnt((size_t)nxcd * nb, 0);
        auto add = [&](int x, int t, int d) {
            cnt[(size_t)x * nb + ta[t]] += d;
            if (tb[t] != ta[t]) cnt[(size_t)x * nb + tb[t]] += d;
        };
        for (int t = 0; t < ntiles; ++t) add(part[t], t, 1);
        auto cost_of = [&]() {
            int c2 = 0;
            for (size_t i = 0; i < cnt.size(); ++i) c2 += cnt[i] > 0;
            return c2;
        };
        // blocks of XCD x in use if tile `out` leaves and tile `in` joins
        auto delta_one = [&](int x, int out, int in) {
            int before = 0, after = 0;
            const int bl[4] = {ta[out], tb[out], ta[in], tb[in]};
            for (int i = 0; i < 4; ++i) {
                bool seen = false;
                for (int j = 0; j < i; ++j) seen = seen || bl[j] == bl[i];
                if (seen) continue;
                const int b = bl[i];
                const int c0 = cnt[(size_t)x * nb + b];
                const int c1 = c0 - ((ta[out] == b) || (tb[out] == b) ? 1 : 0) + ((ta[in] == b) || (tb[in] == b) ? 1 : 0);
                before += c0 > 0;
                after += c1 > 0;
            }
            return after - before;
        };
        uint64_t rng = 0x9E3779B97F4A7C15ull;
        auto next = [&]() {
            rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17;
            return rng;
        };
        int cur = cost_of(), best = cur;
        std::vector<int> best_part = part;
        const int64_t iters = std::min<int64_t>((int64_t)20000 * ntiles, 6000000);  // 0.1 s at F = 4096, 0.3 s at most
        for (int64_t it = 0; it < iters; ++it) {
            const int t1 = (int)(next() % (uint64_t)ntiles), t2 = (int)(next() % (uint64_t)ntiles);
            const int x = part[t1], y = part[t2];
            if (x == y) continue;
            const int d = delta_one(x, t1, t2) + delta_one(y, t2, t1);
            const double temp = 0.4 * (1.0 - (double)it / (double)iters) + 0.05;
            if (d <= 0 || (double)(next() >> 11) / 9007199254740992.0 < exp(-(double)d / temp)) {
                add(x, t1, -1); add(y, t2, -1); add(x, t2, 1); add(y, t1, 1);
                part[t1] = y; part[t2] = x;
                cur += d;
                if (cur < best) { best = cur; best_part = part; }
            }
        }
        part = best_part;
    }
    // launch order: workgroup s * nxcd + x runs on XCD x; an XCD's tiles in (a, b) order, so that neighbours in time share blocks
    std::vector<int> fill(nxcd, 0);
    for (int t = 0; t < ntiles; ++t) map[(size_t)fill[part[t]]++ * nxcd + part[t]] = t;
}

inline void rr_build_tile_map(int nb, int od, int nxcd, std::vector<int> &map) {
    static std::mutex mu;
    static std::map<int, std::vector<int>> cache;  // contexts of one process (device groups, alternating bases) share the maps
    std::lock_guard<std::mutex> lk(mu);
    const int key = (nb * 2 + od) * 64 + nxcd;
    auto it = cache.find(key);
    if (it == cache.end()) {
        std::vector<int> m;
        rr_build_tile_map_uncached(nb, od, nxcd, m);
        it = cache.emplace(key, std::move(m)).first;
    }
    map = it->second;
}
