// wm_sched_probe.cpp - test infrastructure (tests/test_wm_sched.py, tests/test_wm_batch_sched.py): the sweep schedule, the cache
// decision and the block layout of the plain weighted median (primestereomatch_amd/csrc/psm_wm_sched.h) behind a C ABI for ctypes,
// built with the host compiler alone - no context, no device.  The probe plays the device: it is given the counters of all m maps
// (two per pair) as a whole call would leave them, and shows the schedule only what a snapshot behind the sweeps launched so far
// would hold.
// With -DWM_SCHED_PROBE_MAIN it is a program of its own that walks seeded random tables (for a sanitizer build).
#include "../primestereomatch_amd/csrc/psm_wm_sched.h"

#include <algorithm>
#include <cstring>
#include <vector>

using namespace psm;

extern "C" {

int wm_probe_ncnt(void) { return WM_NCNT; }
int wm_probe_cap(void) { return WM_SWEEP_CAP; }
int wm_probe_lane_min(void) { return WM_LANE_MIN; }
int wm_probe_wpix(void) { return WM_WPIX; }

// The driver's loop (wm_sweeps, psm_api_pp.cpp) over `table`: m x WM_NCNT counters.  groups: {begin, end, short form} per group, at
// most max_groups of them; snaps: {slot, extent} per snapshot read; done / tail / sweeps / evals: the schedule's per-map state at
// the end.  Returns the number of groups, n_snaps through its pointer.
int wm_probe_run(const int *table, int m, unsigned flags, int *groups, int max_groups, int *snaps, int *n_snaps, int *done, int *tail, int *sweeps,
                 long long *evals)
{
    WmSched sch(m, flags);
    std::vector<int> pin[2] = {std::vector<int>((size_t)m * WM_NCNT), std::vector<int>((size_t)m * WM_NCNT)};
    int ng = 0, ns = 0;
    auto launch_group = [&](int slot) {
        const WmGroup g = sch.next_group();
        if (ng < max_groups) { groups[3 * ng] = g.begin; groups[3 * ng + 1] = g.end; groups[3 * ng + 2] = g.short_lists; }
        ++ng;
        // the snapshot behind sweep g.end - 1: the counters the sweeps so far have written (sweep k writes its changed count and the
        // next list's length; the seed wrote the first list's), zero beyond
        std::fill(pin[slot].begin(), pin[slot].end(), 0);
        for (int s = 0; s < m; ++s) memcpy(pin[slot].data() + (size_t)s * WM_NCNT, table + (size_t)s * WM_NCNT, (2 * g.end + 1) * sizeof(int));
        sch.launched(g, slot);
    };
    launch_group(0);
    for (int g = 0;; ++g) {
        if (sch.more()) launch_group((g + 1) & 1);
        if (ns < max_groups) { snaps[2 * ns] = g & 1; snaps[2 * ns + 1] = sch.upto[g & 1]; }
        ++ns;
        if (!sch.read(g & 1, pin[g & 1].data())) break;
    }
    *n_snaps = ns;
    for (int s = 0; s < m; ++s) { done[s] = sch.done[s]; tail[s] = sch.tail[s]; sweeps[s] = sch.sweeps[s]; evals[s] = sch.evals[s]; }
    return ng;
}

// -> floats of all sides (0: no cache); need[i]: the floats of side i either way (a pair's right side begins need[left] floats
// into its context's buffer)
unsigned long long wm_probe_cache(const int *n0, int m, unsigned long long avail, unsigned flags, unsigned long long *need)
{
    for (int i = 0; i < m; ++i) need[i] = wm_side_need(n0[i]);
    return wm_cache_plan(n0, m, (size_t)avail, flags);
}

// out = per side the 10 offsets in the order of WmSideAt, then the bytes to allocate: 21 values
void wm_probe_layout(unsigned long long HW, unsigned long long *out)
{
    const WmLayout l = wm_layout((size_t)HW);
    for (int s = 0; s < 2; ++s) {
        const WmSideAt &a = l.s[s];
        const size_t v[10] = {a.orig, a.newv, a.chgb, a.rowany, a.stamp, a.list[0], a.list[1], a.chg, a.slot_of, a.inv};
        for (int i = 0; i < 10; ++i) out[10 * s + i] = v[i];
    }
    out[20] = l.bytes;
}

}  // extern "C"

#ifdef WM_SCHED_PROBE_MAIN
#include <cstdio>
#include <cstdlib>
#include <random>

// Seeded random tables as the tests make them: active counts that fall, a first zero change at a random sweep or none
int main(int argc, char **argv)
{
    const int n = argc > 1 ? atoi(argv[1]) : 4000;
    std::mt19937 rng(12345);
    const int sizes[4] = {2, 4, 6, 16};
    long long total_groups = 0, fall_backs = 0;
    for (int t = 0; t < n; ++t) {
        const int m = sizes[rng() % 4];
        std::vector<int> table((size_t)m * WM_NCNT, 0);
        for (int s = 0; s < m; ++s) {
            int *cnt = table.data() + (size_t)s * WM_NCNT;
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
        const int room = WM_SWEEP_CAP + 8;
        std::vector<int> groups(3 * room), snaps(2 * room), done(m), tail(m), sweeps(m);
        std::vector<long long> evals(m);
        int ns = 0;
        const int ng = wm_probe_run(table.data(), m, flags, groups.data(), room, snaps.data(), &ns, done.data(), tail.data(), sweeps.data(), evals.data());
        if (ng > WM_SWEEP_CAP / 2 || ns > ng) { fprintf(stderr, "table %d: %d groups, %d snapshots\n", t, ng, ns); return 1; }
        total_groups += ng;
        for (int s = 0; s < m; ++s) fall_backs += sweeps[s] < 0;
        std::vector<int> n0(m);
        std::vector<unsigned long long> need(m);
        for (int s = 0; s < m; ++s) n0[s] = (int)(rng() % 100000);
        (void)wm_probe_cache(n0.data(), m, (unsigned long long)rng() << (rng() % 8), flags, need.data());
        unsigned long long out[21];
        wm_probe_layout(81 + rng() % 3000000, out);
    }
    printf("%d tables, %lld groups launched, %lld fall-backs\n", n, total_groups, fall_backs);
    return 0;
}
#endif
