// wm_batch_sched_probe.cpp - test infrastructure (tests/test_wm_batch_sched.py): the sweep schedule and the cache decision of the
// weighted median of several pairs (WmBatchSched, wm_batch_cache_plan; primestereomatch_amd/csrc/psm_wm_sched.h) behind a C ABI for
// ctypes, built with the host compiler alone - no context, no device.  The probe plays the device as tests/wm_sched_probe.cpp does:
// it is given the counters of all m maps as a whole call would leave them, and shows the schedule only what a snapshot behind the
// sweeps launched so far would hold.  The same tables go through WmSched (m = 2) for the comparison.
// With -DWM_BATCH_SCHED_PROBE_MAIN it is a program of its own that walks seeded random tables (for a sanitizer build).
#include "../primestereomatch_amd/csrc/psm_wm_sched.h"

#include <cstring>
#include <vector>

using namespace psm;

namespace {

// S: WmSched (m = 2) or WmBatchSched.  groups: {begin, end, short form} per group, snaps: {slot, extent} per snapshot read;
// done / tail / sweeps / evals: the schedule's per-map state at the end.  Returns the number of groups, n_snaps through its pointer.
template <class S>
int run(S &sch, const int *table, int m, int *groups, int max_groups, int *snaps, int *n_snaps, int *done, int *tail, int *sweeps, long long *evals)
{
    std::vector<int> pin[2] = {std::vector<int>((size_t)m * WM_NCNT), std::vector<int>((size_t)m * WM_NCNT)};
    int ng = 0, ns = 0;
    auto launch_group = [&](int slot) {
        const WmGroup g = sch.next_group();
        if (ng < max_groups) { groups[3 * ng] = g.begin; groups[3 * ng + 1] = g.end; groups[3 * ng + 2] = g.short_lists; }
        ++ng;
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

}  // namespace

extern "C" {

int wmb_probe_ncnt(void) { return WM_NCNT; }
int wmb_probe_cap(void) { return WM_SWEEP_CAP; }
int wmb_probe_lane_min(void) { return WM_LANE_MIN; }
int wmb_probe_wpix(void) { return WM_WPIX; }

// table: m x WM_NCNT counters
int wmb_probe_run(const int *table, int m, unsigned flags, int *groups, int max_groups, int *snaps, int *n_snaps, int *done, int *tail, int *sweeps,
                  long long *evals)
{
    WmBatchSched sch(m, flags);
    return run(sch, table, m, groups, max_groups, snaps, n_snaps, done, tail, sweeps, evals);
}

// the same through the single pair's schedule (m = 2)
int wmb_probe_run_single(const int *table, unsigned flags, int *groups, int max_groups, int *snaps, int *n_snaps, int *done, int *tail, int *sweeps,
                         long long *evals)
{
    WmSched sch(flags);
    return run(sch, table, 2, groups, max_groups, snaps, n_snaps, done, tail, sweeps, evals);
}

// -> floats of all sides (0: no cache); need[i]: the floats of side i either way
unsigned long long wmb_probe_cache(const int *n0, int m, unsigned long long avail, unsigned flags, unsigned long long *need)
{
    for (int i = 0; i < m; ++i) need[i] = wm_side_need(n0[i]);
    return wm_batch_cache_plan(n0, m, (size_t)avail, flags);
}

// the single pair's decision: floats of both sides (0: none)
unsigned long long wmb_probe_cache_single(int n0l, int n0r, unsigned long long avail, unsigned flags)
{
    const int n0[2] = {n0l, n0r};
    return wm_cache_plan(n0, (size_t)avail, flags).floats;
}

}  // extern "C"

#ifdef WM_BATCH_SCHED_PROBE_MAIN
#include <cstdio>
#include <cstdlib>
#include <random>

// Seeded random tables as the test makes them: active counts that fall, a first zero change at a random sweep or none
int main(int argc, char **argv)
{
    const int n = argc > 1 ? atoi(argv[1]) : 2000;
    std::mt19937 rng(4321);
    const int sizes[4] = {2, 4, 6, 16};
    long long total_groups = 0, fall_backs = 0;
    for (int t = 0; t < n; ++t) {
        const int m = sizes[rng() % 4];
        std::vector<int> table((size_t)m * WM_NCNT, 0);
        for (int s = 0; s < m; ++s) {
            int *cnt = table.data() + (size_t)s * WM_NCNT;
            int act = (int)(rng() % 40000);
            const int stop = rng() % 4 ? (int)(rng() % (WM_SWEEP_CAP + 4)) : -1;
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
        const int ng = wmb_probe_run(table.data(), m, flags, groups.data(), room, snaps.data(), &ns, done.data(), tail.data(), sweeps.data(), evals.data());
        if (ng > WM_SWEEP_CAP / 2 || ns > ng) { fprintf(stderr, "table %d: %d groups, %d snapshots\n", t, ng, ns); return 1; }
        if (m == 2) {
            std::vector<int> g1(3 * room), s1(2 * room), d1(2), t1(2), w1(2);
            std::vector<long long> e1(2);
            int ns1 = 0;
            const int ng1 = wmb_probe_run_single(table.data(), flags, g1.data(), room, s1.data(), &ns1, d1.data(), t1.data(), w1.data(), e1.data());
            if (ng1 != ng || ns1 != ns || g1 != groups || s1 != snaps || d1 != done || t1 != tail || w1 != sweeps || e1 != evals) {
                fprintf(stderr, "table %d: the batch schedule of two maps differs from the single pair's\n", t);
                return 1;
            }
        }
        total_groups += ng;
        for (int s = 0; s < m; ++s) fall_backs += sweeps[s] < 0;
        std::vector<int> n0(m);
        std::vector<unsigned long long> need(m);
        for (int s = 0; s < m; ++s) n0[s] = (int)(rng() % 100000);
        (void)wmb_probe_cache(n0.data(), m, (unsigned long long)rng() << (rng() % 8), flags, need.data());
    }
    printf("%d tables, %lld groups launched, %lld fall-backs\n", n, total_groups, fall_backs);
    return 0;
}
#endif
