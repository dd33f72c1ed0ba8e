// wm_sched_probe.cpp - test infrastructure (tests/test_wm_sched.py): the sweep schedule, the cache decision and the block layout
// of the plain weighted median (primestereomatch_amd/csrc/psm_wm_sched.h) behind a C ABI for ctypes, built with the host compiler
// alone - no context, no device.  The probe plays the device: it is given the counters of both maps as a whole call would leave
// them, and shows the schedule only what a snapshot behind the sweeps launched so far would hold.
// With -DWM_SCHED_PROBE_MAIN it is a program of its own that walks seeded random tables (for a sanitizer build).
#include "../primestereomatch_amd/csrc/psm_wm_sched.h"

#include <cstring>

using namespace psm;

extern "C" {

int wm_probe_ncnt(void) { return WM_NCNT; }
int wm_probe_cap(void) { return WM_SWEEP_CAP; }
int wm_probe_lane_min(void) { return WM_LANE_MIN; }
int wm_probe_wpix(void) { return WM_WPIX; }

// The driver's loop (psm_wgt_median) over `table`: 2 x WM_NCNT counters.  launches: {sweep, short form} per launched sweep, at most
// max_launches of them; snaps: {slot, extent} per snapshot read; out: {sweeps L, sweeps R}, evals: {L, R}.  Returns the number
// of launches, n_snaps through its pointer.
int wm_probe_run(const int *table, unsigned flags, int *launches, int max_launches, int *snaps, int *n_snaps, int *sweeps, long long *evals)
{
    WmSched sch(flags);
    int pin[2][2 * WM_NCNT];
    int nl = 0, ns = 0;
    auto launch_group = [&](int slot) {
        const WmGroup g = sch.next_group();
        for (int sw = g.begin; sw < g.end; ++sw, ++nl)
            if (nl < max_launches) { launches[2 * nl] = sw; launches[2 * nl + 1] = g.short_lists; }
        // the snapshot behind sweep g.end - 1: the counters the sweeps so far have written (sweep k writes its changed count and the
        // next list's length; the seed wrote the first list's), zero beyond
        memset(pin[slot], 0, sizeof pin[slot]);
        for (int s = 0; s < 2; ++s) memcpy(pin[slot] + s * WM_NCNT, table + s * WM_NCNT, (2 * g.end + 1) * sizeof(int));
        sch.launched(g, slot);
    };
    launch_group(0);
    for (int g = 0;; ++g) {
        if (sch.more()) launch_group((g + 1) & 1);
        snaps[2 * ns] = g & 1; snaps[2 * ns + 1] = sch.upto[g & 1]; ++ns;
        if (!sch.read(g & 1, pin[g & 1])) break;
    }
    *n_snaps = ns;
    for (int s = 0; s < 2; ++s) { sweeps[s] = sch.sweeps[s]; evals[s] = sch.evals[s]; }
    return nl;
}

// out = {floats of the cache (0: none), the right side's first float}
void wm_probe_cache(int n0l, int n0r, unsigned long long avail, unsigned flags, unsigned long long *out)
{
    const int n0[2] = {n0l, n0r};
    const WmCachePlan p = wm_cache_plan(n0, (size_t)avail, flags);
    out[0] = p.floats; out[1] = p.right;
}

// out = per side the 11 offsets in the order of WmSideAt, then {counter block, bytes, ints per snapshot}: 25 values
void wm_probe_layout(unsigned long long HW, unsigned long long *out)
{
    const WmLayout l = wm_layout((size_t)HW);
    for (int s = 0; s < 2; ++s) {
        const WmSideAt &a = l.s[s];
        const size_t v[11] = {a.orig, a.newv, a.chgb, a.rowany, a.stamp, a.list[0], a.list[1], a.chg, a.slot_of, a.inv, a.cnt};
        for (int i = 0; i < 11; ++i) out[11 * s + i] = v[i];
    }
    out[22] = l.cnt; out[23] = l.bytes; out[24] = l.snap;
}

}  // extern "C"

#ifdef WM_SCHED_PROBE_MAIN
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

// Seeded random tables as the test makes them: active counts that fall, a first zero change at a random sweep or none
int main(int argc, char **argv)
{
    const int n = argc > 1 ? atoi(argv[1]) : 4000;
    std::mt19937 rng(12345);
    long long total_launches = 0, fall_backs = 0;
    for (int t = 0; t < n; ++t) {
        std::vector<int> table(2 * WM_NCNT, 0);
        for (int s = 0; s < 2; ++s) {
            int *cnt = table.data() + s * WM_NCNT;
            int act = (int)(rng() % 40000);
            const int stop = rng() % 4 ? (int)(rng() % (WM_SWEEP_CAP + 4)) : -1;      // (beyond the cap: never seen)
            for (int k = 0; k <= WM_SWEEP_CAP; ++k) {
                cnt[2 * k] = act;
                if (k == WM_SWEEP_CAP) break;
                const bool fixed = k == stop || act == 0;
                cnt[2 * k + 1] = fixed ? 0 : 1 + (int)(rng() % (unsigned)act);
                act = fixed ? 0 : (int)(rng() % (unsigned)(act + 1));
            }
        }
        const unsigned flags = rng() % 8 ? 0u : (unsigned)PSM_FLAG_WMF_TWO_SWEEPS;
        std::vector<int> launches(2 * (WM_SWEEP_CAP + 8)), snaps(2 * (WM_SWEEP_CAP + 8));
        int ns = 0, sweeps[2];
        long long evals[2];
        const int nl = wm_probe_run(table.data(), flags, launches.data(), WM_SWEEP_CAP + 8, snaps.data(), &ns, sweeps, evals);
        if (nl > WM_SWEEP_CAP || ns > nl) { fprintf(stderr, "table %d: %d launches, %d snapshots\n", t, nl, ns); return 1; }
        total_launches += nl;
        fall_backs += (sweeps[0] < 0) + (sweeps[1] < 0);
        unsigned long long out[25];
        wm_probe_cache((int)(rng() % 100000), (int)(rng() % 100000), (unsigned long long)rng() << (rng() % 8), flags, out);
        wm_probe_layout(81 + rng() % 3000000, out);
    }
    printf("%d tables, %lld sweeps launched, %lld fall-backs\n", n, total_launches, fall_backs);
    return 0;
}
#endif
