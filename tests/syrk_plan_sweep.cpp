// The Gram launchers' planner (revrand_amd/csrc/rr_syrk_plan.h) over a sweep of shapes, CU counts and modes: every plan
// without an error must satisfy what the kernels rely on.  Host compiler only, built with
// -fsanitize=address,undefined -fno-sanitize-recover=all and run directly (tests/test_syrk_plan_host.py).
#include "rr_syrk_plan.h"

static long long failures = 0;

#define HOLD(cond)                                                                                                          \
    do {                                                                                                                    \
        if (!(cond) && ++failures <= 20)                                                                                    \
            printf("FAILED %s: %s rows %lld F %d flag %d det %d cu %d\n", #cond, what, (long long)rows, F, flag, det, cu);   \
    } while (0)

// kb: the kernels' k-block; max_rps: the f32 accumulation's row limit per K-split (0: none, the f64 pair)
static void check(const char *what, const SyrkPlan &p, int64_t rows, int F, int flag, int det, int cu, int kb, int64_t max_rps) {
    if (p.err) {
        HOLD(p.msg[0] != 0);
        return;
    }
    const SyrkLaunch *l[3] = {&p.off, &p.ragged, &p.diag};
    int launched = 0;
    for (int i = 0; i < 3; ++i) {
        if (!l[i]->kernel) continue;
        ++launched;
        HOLD(l[i]->nsplit >= 1);
        HOLD(l[i]->nsplit * l[i]->rps >= rows);
        HOLD(l[i]->rps > 0 && l[i]->rps % kb == 0);
        HOLD(max_rps == 0 || l[i]->rps <= max_rps);
        HOLD(l[i]->grid >= 1 && l[i]->grid < (int64_t)1 << 31);
        HOLD(!det || l[i]->rps == p.off.rps);
        HOLD(!det || l[i]->nsplit == p.slabs);
    }
    HOLD(launched >= 1 && p.off.kernel != SK_NONE);
    HOLD(p.route != SR_MERGED || p.off.grid + p.diag.grid < (int64_t)1 << 31);
    HOLD(!p.use_map || p.ntiles % 8 == 0);
    HOLD((p.slabs > 0) == (det != 0));
}

int main() {
    const int64_t ROWS[] = {1, 31, 32, 33, 255, 256, 1023, 1024, 1025, 32767, 32768, 32769, 44484, 1000003, (int64_t)1 << 21,
                            (int64_t)1 << 25};
    const int FS[] = {1, 255, 256, 257, 448, 449, 512, 1024, 1025, 1216, 1217, 4096, 4100, 16384};
    const int CUS[] = {1, 8, 64, 104, 256, 304};
    const SyrkSwitches sw = rr_syrk_switches();  // no switch set: the test clears them
    long long plans = 0;
    for (int64_t rows : ROWS)
        for (int F : FS)
            for (int cu : CUS)
                for (int flag = 0; flag < 2; ++flag)
                    for (int det = 0; det < 2; ++det) {
                        const int64_t ld256 = ((int64_t)F + 255) / 256 * 256, ld128 = ((int64_t)F + 127) / 128 * 128;
                        check("f32", rr_plan_syrk_f32(rows, ld256, F, flag, cu, det, sw), rows, F, flag, det, cu, 32, 32768);
                        check("f64", rr_plan_syrk_f64(rows, ld128, F, flag, cu, det, sw), rows, F, flag, det, cu, 16, 0);
                        plans += 2;
                        if (det) continue;  // the split engines have no deterministic mode
                        check("split16", rr_plan_syrk_split16(rows, ld256, F, flag, cu, sw), rows, F, flag, 0, cu, 64, flag ? 16384 : 32768);
                        ++plans;
                    }
    // the posterior's square, lower triangular operands
    for (int64_t n : {128, 512, 1024, 2048, 4096})
        for (int cu : CUS) {
            const int64_t rows = n;
            const int F = (int)n, flag = 1, det = 0;
            check("f64 square", rr_plan_syrk_f64(n, n, F, 1, cu, 0, sw), rows, F, flag, det, cu, 16, 0);
            ++plans;
        }
    // the tile maps the plans ask for: a permutation of the tiles
    for (int nb : {2, 5, 16, 17})
        for (int od = 0; od < 2; ++od) {
            const int ntiles = od ? nb * (nb - 1) / 2 : nb * (nb + 1) / 2;
            if (ntiles % SYRK_NXCD) continue;
            std::vector<int> map, count(ntiles, 0);
            rr_build_tile_map(nb, od, SYRK_NXCD, map);
            bool ok = (int)map.size() == ntiles;
            for (int t : map) ok = ok && t >= 0 && t < ntiles && ++count[t] == 1;
            if (!ok && ++failures) printf("FAILED tile map nb %d od %d\n", nb, od);
        }
    printf("%lld plans %s, %lld failures\n", plans, failures ? "checked" : "hold", failures);
    return failures ? 1 : 0;
}
