// psm_state.h - what a context (psm_ctx.h) remembers between two calls of the C ABI about its cost volumes, its results and its image
// pairs: plain records, the questions the entry points ask of them and the only functions that change them.  Nothing of HIP in here: it
// compiles with the host compiler alone (tests/test_ctx_state.py walks the transitions that way).
#pragma once
#include <cstdint>

namespace psm {

// A range of image rows [y0, y1); empty (y1 <= y0): no row.
struct Rows {
    int y0 = 0, y1 = 0;
    bool empty() const { return y1 <= y0; }
    bool covers(Rows need) const { return need.empty() || (y0 <= need.y0 && y1 >= need.y1); }
    bool operator==(Rows o) const { return y0 == o.y0 && y1 == o.y1; }
};
inline Rows whole_image(int H) { return Rows{0, H}; }

// ---- What stands for vol[side] ----
// Two facts: whether the UNFILTERED costs are a recipe (built inside the fused kernel from the g1 planes, never written), and in
// which form a FILTERED result is waiting for its reader.  Five combinations exist:
//   lazy   pending
//   yes    NOTHING   costs are a recipe; nothing filtered yet
//   no     NOTHING   vol[side] holds real data (costs, or a filtered volume: the library does not tell them apart)
//   yes    KEYS      filtered result = the packed minima in keys_cur (the select forms of the fused kernel); costs still a recipe
//   no     KEYS      the same; vol[side] still holds the UNFILTERED costs
//   no     FGF       filtered result = the low-resolution models fgf_mab[side] of psm_cost_filter_fgf (sub: its subsample rate).
//                    vol[side] "stands for" it and counts as not lazy although it may not even be allocated: every reader
//                    but the WTA flushes the models into it first (fgf_flush allocates)
// Keys and models exclude each other, and models leave no recipe behind: the functions below cannot write anything else.
struct VolSide {
    enum Pending { NOTHING, KEYS, FGF };
    bool lazy = false; Pending pending = NOTHING; int sub = 0;
};
inline bool costs_lazy(const VolSide &v) { return v.lazy; }
inline bool pending_keys(const VolSide &v) { return v.pending == VolSide::KEYS; }
inline int pending_fgf(const VolSide &v) { return v.pending == VolSide::FGF ? v.sub : 0; }            // the subsample rate, or 0
inline bool all_real(const VolSide &v) { return !v.lazy && v.pending == VolSide::NOTHING; }           // everything of the side is memory
inline bool fresh_lazy(const VolSide &v) { return v.lazy && v.pending == VolSide::NOTHING; }          // as a lazy CostConst leaves it
inline void new_costs(VolSide &v, bool lazy) { v = VolSide{lazy, VolSide::NOTHING, 0}; }                // ... replace whatever was there or pending
inline void costs_built(VolSide &v) { v.lazy = false; }                                                 // the recipe was carried out into vol[side]
inline void filtered_to_keys(VolSide &v) { v.pending = VolSide::KEYS; v.sub = 0; }                      // the costs stay what they were
inline void filtered_to_fgf(VolSide &v, int sub) { v = VolSide{false, VolSide::FGF, sub}; }
inline void in_memory(VolSide &v) { v = VolSide{}; }                                                    // filtered into vol[side], models flushed, volume uploaded

// ---- The current results ----
struct Results {
    bool maps = false, mask = false;    // the map buffer holds the maps of the current frame; `valid` their L-R mask (never without the maps)
    bool keys[2] = {false, false};      // keys_cur holds the side's packed minima over the local slices (psm_disp_select_partial*)
    // The rows the minima and the maps cover: the psm_set_rows stripe in force when psm_cost_filter produced them - recorded at
    // filter time, psm_set_rows itself only affects the NEXT filter - else the whole image ([0, H) from psm_create* on).
    Rows rows;
    // The rows the last filter covered, as it recorded them: `rows` follows whoever wrote the maps last (an upload, the SGM stage, a
    // gather cover the whole image), the pending minima go on covering these - a select of them brings `rows` back here.
    Rows filt;
    const uint8_t *early = nullptr;     // the map buffer the single-phase filter's reduction (k_chunk_min) already filled, or null
};
inline void maps_gone(Results &r) { r.maps = r.mask = false; }
inline void forget_early(Results &r) { r.early = nullptr; }
inline void stale(Results &r) { maps_gone(r); forget_early(r); }            // new costs, a volume uploaded
// ... or a filter ran, for `rows`; early: the map buffer its own reduction filled on the way (null: none)
inline void filtered(Results &r, Rows rows, const uint8_t *early) { maps_gone(r); r.rows = r.filt = rows; r.early = early; }
inline void cover(Results &r, Rows rows) { r.rows = rows; }
inline void cover_filtered(Results &r) { r.rows = r.filt; }               // what is selected from the pending minima covers what they cover
inline void maps_written(Results &r) { r.maps = true; r.mask = false; }     // new maps: a mask of earlier ones does not describe them
inline void mask_written(Results &r) { r.mask = r.maps; }
// psm_disp_select, both sides pending as keys: true when `maps` is what the filter's reduction filled - once
inline bool take_early(Results &r, const uint8_t *maps) { const bool hit = r.early == maps; r.early = nullptr; return hit; }
inline void keys_complete(Results &r, int side) { r.keys[side] = true; }
inline void keys_gone(Results &r) { r.keys[0] = r.keys[1] = false; }

// ---- The image pair and the one on its way ----
// The bookkeeping of psm::PairSlots (psm_ctx.h) that needs no device.  Depths are PSM_IMG_* (-1: no such pair).  The staged pair
// lies in the second image slot until the next psm_cost_construct adopts it; a blocking upload in between supersedes it.
// depth, next_depth: of the current pair / of the staged one; slot: the page-locked staging slot the last asynchronous upload filled;
// range_pending: the staged pair's measured range is still on its way (float pairs); inside: the current pair lies inside the select
// forms' domain (psm_ctx.h: scaled_forms_ok).
struct PairState {
    int depth = -1, next_depth = -1, slot = 0;
    bool range_pending = false, inside = true;
};
inline bool pair_staged(const PairState &p) { return p.next_depth >= 0; }
inline int depth_at_construct(const PairState &p) { return pair_staged(p) ? p.next_depth : p.depth; }   // ... the next psm_cost_construct will find
inline int next_slot(PairState &p) { return p.slot ^= 1; }                                              // 1, 0, 1, ...
inline void uploaded(PairState &p, int depth, bool inside) { p.depth = depth; p.inside = inside; p.next_depth = -1; p.range_pending = false; }   // blocking
inline void staged(PairState &p, int depth, bool range_pending) { p.next_depth = depth; p.range_pending = range_pending; }   // replaces a pair staged before; (-1, false): gives it up; (its depth, false): its range has arrived
inline void adopted(PairState &p, bool inside) { if (pair_staged(p)) uploaded(p, p.next_depth, inside); }   // nothing staged: nothing happens

}  // namespace psm
