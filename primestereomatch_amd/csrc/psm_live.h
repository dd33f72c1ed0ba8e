// psm_live.h - which (column group, slice) work items of the select forms of k_cvf_pc can change the result.  Plain C++ without
// a HIP dependency: the planner's item table (pc_live), k_cvf_pc and a CPU test (through psm_debug_pc_dead) all call these
// functions; k_chunk_min reads the chunks that table names.
//
// The costs are built on the fly.  A voxel of the left volume takes the d-invariant border cost where its input column c has no
// partner, c < d; a voxel of the right volume where c >= W - d (src/CVC.cpp:135-146,165-176; 8-bit mode: the other image reads
// as 255 there).  The guided filter is two 8-tap box filters anchored at 4, each with its own REFLECT_101 (src/CVF.cpp:72-165):
//   output column x   reads model columns r101(x-4) .. r101(x+3),
//   model column m    reads input columns r101(m-4) .. r101(m+3),
// and the guidance, the border cost and every rounding are functions of the pixel, not of d.  Once EVERY input column under an
// output column is a border column, the filtered slice holds the same bits there for every larger d:
//   left:   the largest input column is x+6 (no reflection: x+3, then +3), a border column when x+6 < d: from d = x+7 on.
//           At the image's left edge the reflection reaches further: x = 0 reads model column r101(-4) = 4, which reads input
//           column 7 - from d = 8 on (x = 1: model column 4 again, 8 = x+7; no exception from there).  At the right edge the
//           reflected columns lie below x+6.
//   right:  the smallest input column is x-8 (x-4, then -4), a border column when x-8 >= W-d: from d = W-x+8 = x'+9 on,
//           x' = W-1-x the distance from the right edge.  Reflections only reach columns above x-8: no exception.
// DispSel::CVSelect takes the lowest d on ties (src/DispSel.cpp:96-104), so a slice whose next lower slice of the same context
// already lies in that constant region - in every column of the group - can never win: it is dead.  So is d = 0, never a
// candidate.  A context's first slice is never dead by this rule, whatever its d: it carries the constant value.
#pragma once

#if defined(__HIPCC__)
#define PSM_LIVE_FN __host__ __device__ inline
#else
#define PSM_LIVE_FN inline
#endif

namespace psm {

// first d from which every output column xfirst .. xlast of a volume repeats the slice below it (see above)
PSM_LIVE_FN int pc_border_from(int right, int xfirst, int xlast, int W)
{
    if (xlast > W - 1) xlast = W - 1;
    if (right) return (W - 1 - xfirst) + 9;
    const int t = xlast + 7;
    return xfirst <= 0 && t < 8 ? 8 : t;          // (a group of column 0 alone: the reflected window, see above)
}

// The liveness predicate.  Slice with global disparity dg of the volume `right` (0: left), output columns xfirst .. xlast;
// dprev: the next lower global disparity this context owns (both launches of a two-phase selection together), < 0: none.
PSM_LIVE_FN bool pc_dead(int right, int xfirst, int xlast, int W, int dg, int dprev)
{
    if (dg == 0) return true;
    return dprev >= 0 && dprev >= pc_border_from(right, xfirst, xlast, W);
}

// Slice j of a launch -> local slice of the context.  sel 0: all slices; 1: every step-th; 2: the others (PcSel).
PSM_LIVE_FN int pc_sel_index(int sel, int step, int j)
{
    return sel == 1 ? j * step : (sel == 2 ? (j / (step - 1)) * step + j % (step - 1) + 1 : j);
}

// Which slices a context owns (local slice i = global disparity d_begin + i * dstep) and which of them a launch covers.
struct PcOwn {
    int on;               // 0: nothing is skipped (costs read from memory, the storing form, one-volume launches)
    int d_begin, dstep;
    int sel, step;
};

// the predicate for slice j of a launch
PSM_LIVE_FN bool pc_dead_at(const PcOwn &o, int right, int xfirst, int xlast, int W, int j)
{
    if (!o.on) return false;
    const int i = pc_sel_index(o.sel, o.step, j);
    return pc_dead(right, xfirst, xlast, W, o.d_begin + i * o.dstep, i > 0 ? o.d_begin + (i - 1) * o.dstep : -1);
}

// Deadness by the border rule is monotone in d: of a launch's n slices in ascending order the first pc_live_end are left
// (closed form of the predicate; pc_live checks it against pc_dead_at at the boundary, the CPU test everywhere).
PSM_LIVE_FN int pc_live_end(const PcOwn &o, int right, int xfirst, int xlast, int W, int n)
{
    if (!o.on) return n;
    const int t = pc_border_from(right, xfirst, xlast, W);
    // local slice i >= 1 is dead when d_begin + (i-1) * dstep >= t: from i = ilim on
    const int ilim = o.d_begin >= t ? 1 : 1 + (t - o.d_begin + o.dstep - 1) / o.dstep;
    // launch slices j with pc_sel_index(j) < ilim
    const int below = o.sel == 1 ? (ilim + o.step - 1) / o.step : (o.sel == 2 ? ilim - (ilim + o.step - 1) / o.step : ilim);
    return below < n ? below : n;
}

}  // namespace psm
