// psm_wm_sched.h - what the host driver of the plain weighted median (pp_enqueue, psm_api_pp.cpp) decides without
// the device, for the maps of one pair or of several: where the parts of a context's sweep block lie, what the per-sweep counters
// mean, how many sweeps the next group holds and in which form, when a map is finished, and whether the call gets a weight cache.
// Nothing of HIP in here: it compiles with the host compiler alone (tests/test_wm_sched.py and tests/test_wm_batch_sched.py play
// the device to it through tests/wm_sched_probe.cpp).
#pragma once
#include "../../include/primesm_hip.h"

#include <cstddef>
#include <cstdint>
#include <vector>

namespace psm {

constexpr int WM_LANE_MIN = 8192;       // active pixels from which a sweep evaluates one pixel per LANE (k_wm_eval) instead of per wave
constexpr int WM_WROW = 20;             // floats per window row of the weight cache (19 weights + 1 pad: five float4)
constexpr int WM_WPIX = 19 * WM_WROW;   // floats per cached pixel
constexpr int WM_SWEEP_CAP = 96;        // sweeps of the parallel form before a map falls back to the dataflow form
constexpr int WM_NCNT = 2 * (WM_SWEEP_CAP + 2);   // counters per map

// ---- The counters of one map (WmSide::cnt, psm_kernels.h): sweep k evaluates wm_active(cnt, k) pixels, changes wm_changed(cnt, k)
// of them and leaves a list of wm_next(cnt, k) for sweep k + 1; wm_active(cnt, 0) is the number of invalid pixels.
inline int wm_active(const int *cnt, int k) { return cnt[2 * k]; }
inline int wm_changed(const int *cnt, int k) { return cnt[2 * k + 1]; }
inline int wm_next(const int *cnt, int k) { return cnt[2 * k + 2]; }
// ... of map s in a snapshot of the counter block (all maps of the call, one behind the other)
inline const int *wm_counters(const int *snap, int s) { return snap + s * WM_NCNT; }

// ---- The sweep block of a context: byte offsets from its base.  Per side orig, newv, chgb, rowany (nb bytes each), then stamp, the two
// active lists, the changed list, slot_of and the list of all invalid pixels (nb ints each), nb = W H rounded up to 256.  (The
// counters are not in it: those of all maps of a call lie in one block of the call's first context, psm::WmBatch.)
struct WmSideAt { size_t orig, newv, chgb, rowany, stamp, list[2], chg, slot_of, inv; };
struct WmLayout {
    WmSideAt s[2];
    size_t bytes;          // to allocate
};
inline WmLayout wm_layout(size_t HW)
{
    const size_t nb = (HW + 255) / 256 * 256, per_side = 4 * nb + 6 * nb * sizeof(int);
    WmLayout l;
    l.bytes = 2 * per_side;
    for (int s = 0; s < 2; ++s) {
        const size_t b = s * per_side, ip = b + 4 * nb;
        auto ints = [&](int i) { return ip + i * nb * sizeof(int); };
        l.s[s] = WmSideAt{b, b + nb, b + 2 * nb, b + 3 * nb, ints(0), {ints(1), ints(2)}, ints(3), ints(4), ints(5)};
    }
    return l;
}

// ---- The schedule of the m = 2 n maps of a call (n = 1: a single pair), map 2 i + s being side s of pair i; their counters lie one
// behind the other in one block (wm_counters(snap, map)), so one snapshot shows them all.  Sweeps are launched in groups; the host
// looks at a group's counters (did a sweep change nothing? how long is the next list?) while the NEXT group is already queued - the
// device never idles behind a host round trip (~65 us of idle per check, 0.7 ms of the 4.0 on the 1080p bench pair).  A group
// launched for a map that had already reached its fixed point is a handful of launches over empty lists.  A launch takes every
// map one way: a group is of the one-launch wave form only when EVERY map is tail or done, and the loop ends when every map is
// done or the cap is reached.  The driver's loop:
//     launched(next_group(), 0);
//     for (g = 0;; ++g) { if (more()) launched(next_group(), (g + 1) & 1);  if (!read(g & 1, snapshot of slot g & 1)) break; }
struct WmGroup { int begin, end; bool short_lists; };      // sweeps [begin, end); short_lists: the one-launch wave form
struct WmSched {
    int cap;                            // WM_SWEEP_CAP; 2 under PSM_FLAG_WMF_TWO_SWEEPS (test hook for the fall-back)
    int m;                              // maps
    int sw = 0;                         // sweeps launched
    int unread = 0;                     // groups launched whose snapshot has not been read
    int upto[2] = {0, 0};               // sweeps covered by the snapshot in a slot
    std::vector<char> done;             // the map has reached its fixed point
    std::vector<char> tail;             // the list going into the next sweep is short: one launch per sweep, more sweeps per check
    std::vector<int> sweeps;            // what psm_wgt_median_stats reports; as initialised (-1): a map left to the dataflow form
    std::vector<long long> evals;

    WmSched(int maps, unsigned flags)
        : cap((flags & PSM_FLAG_WMF_TWO_SWEEPS) ? 2 : WM_SWEEP_CAP), m(maps), done(maps, 0), tail(maps, 0), sweeps(maps, -1), evals(maps, 0) {}
    bool more() const { return sw < cap; }
    bool all_done() const
    {
        for (int i = 0; i < m; ++i)
            if (!done[i]) return false;
        return true;
    }
    // two sweeps per group while the lists are long (the host learns two groups late that they have become short, and a sweep
    // launched the long way costs three launches more than it needs then), eight once they are short
    WmGroup next_group() const
    {
        bool short_lists = true;
        for (int i = 0; i < m; ++i) short_lists = short_lists && (tail[i] || done[i]);
        const int chk = short_lists ? 8 : 2;
        return WmGroup{sw, sw + chk < cap ? sw + chk : cap, short_lists};
    }
    void launched(const WmGroup &g, int slot) { sw = g.end; upto[slot] = sw; ++unread; }
    // snap: the counters of all m maps behind the group of `slot`; false when every map is finished or nothing more is queued
    bool read(int slot, const int *snap)
    {
        const int seen = upto[slot];
        for (int i = 0; i < m; ++i) {
            if (done[i]) continue;
            const int *cnt = wm_counters(snap, i);
            long long ev = 0;
            for (int k = 0; k < seen; ++k) {
                ev += wm_active(cnt, k);
                if (wm_changed(cnt, k) == 0) {      // sweep k changed nothing: fixed point
                    done[i] = 1;
                    sweeps[i] = k + 1;
                    evals[i] = ev;
                    break;
                }
            }
            tail[i] = seen < cap && wm_next(cnt, seen - 1) < WM_LANE_MIN;   // (what the group's last sweep left for the next one: wave form)
        }
        return --unread > 0 && !all_done();
    }
};

// ---- The weight cache: the 19 x 19 weights of an invalid pixel depend on the image only, and the sweeps evaluate it ~5 times.  One
// pass forms them all (1.5 KB per invalid pixel: wm_side_need floats per side, whole blocks of 64 pixels - the cache is laid out in
// such blocks); short lists form their weights themselves.  The decision is one for all m maps of a call, since a launch takes
// every map one way: cached only if at least one side has WM_LANE_MIN invalid pixels, the sum of all sides' needs stays within the
// bound and no flag forbids it - then EVERY side gets its weights, a context's two sides one behind the other in its own buffer
// (the right side's begin wm_side_need(n0[left]) floats into it).  n0: the invalid pixels of the m maps; avail: the bytes the device
// has free plus what the contexts' caches hold already (SIZE_MAX: unknown).  At most 12 GB, and never more than half of avail: the
// volumes, the spare volume and the FGF scratch of this or another context on the device are allocated on first use and must still
// fit.  The maps are the same either way.  Returns the floats of all sides, 0: no cache.
inline size_t wm_side_need(int n0) { return (size_t)((n0 + 63) / 64 * 64) * WM_WPIX; }
inline size_t wm_cache_plan(const int *n0, int m, size_t avail, unsigned flags)
{
    size_t max_bytes = (size_t)12 << 30;
    if (avail / 2 < max_bytes) max_bytes = avail / 2;
    size_t tot = 0;
    bool any = false;
    for (int i = 0; i < m; ++i) {
        tot += wm_side_need(n0[i]);
        any = any || n0[i] >= WM_LANE_MIN;
    }
    const bool none = !any || tot * sizeof(float) > max_bytes || (flags & PSM_FLAG_WMF_NO_CACHE);
    return none ? 0 : tot;
}

}  // namespace psm
