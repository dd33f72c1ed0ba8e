// ctx_state_probe.cpp - test infrastructure (tests/test_ctx_state.py): the records of primestereomatch_amd/csrc/psm_state.h and
// their transitions behind a C ABI for ctypes, built with the host compiler alone - no context, no device.
#include "../primestereomatch_amd/csrc/psm_state.h"

using namespace psm;

extern "C" {

// One transition of a volume side.  st = {lazy, pending, sub} in and out; returns the answers to the five questions as bits.
int side_step(int *st, int op, int arg)
{
    VolSide v{st[0] != 0, (VolSide::Pending)st[1], st[2]};
    switch (op) {
    case 0: new_costs(v, arg != 0); break;
    case 1: costs_built(v); break;
    case 2: filtered_to_keys(v); break;
    case 3: filtered_to_fgf(v, arg); break;
    case 4: in_memory(v); break;
    default: break;                       // (the questions of the state as it is)
    }
    st[0] = v.lazy; st[1] = v.pending; st[2] = v.sub;
    return costs_lazy(v) | pending_keys(v) << 1 | (pending_fgf(v) != 0) << 2 | all_real(v) << 3 | fresh_lazy(v) << 4 |
           (pending_fgf(v) == (v.pending == VolSide::FGF ? v.sub : 0)) << 5;
}

// One transition of the results.  st = {maps, mask, keys L, keys R, y0, y1, early} in and out, early: 0 = none, n = map buffer n.
int res_step(int *st, int op, int a, int b, int e)
{
    static const uint8_t buf[8] = {};
    Results r;
    r.maps = st[0]; r.mask = st[1]; r.keys[0] = st[2]; r.keys[1] = st[3]; r.rows = Rows{st[4], st[5]}; r.early = st[6] ? buf + st[6] : nullptr;
    int ret = 0;
    switch (op) {
    case 0: stale(r); break;
    case 1: filtered(r, Rows{a, b}, e ? buf + e : nullptr); break;
    case 2: cover(r, Rows{a, b}); break;
    case 3: maps_written(r); break;
    case 4: mask_written(r); break;
    case 5: ret = take_early(r, buf + e); break;
    case 6: forget_early(r); break;
    case 7: maps_gone(r); break;
    case 8: keys_complete(r, a); break;
    case 9: keys_gone(r); break;
    default: r = Results{}; break;        // a new record
    }
    st[0] = r.maps; st[1] = r.mask; st[2] = r.keys[0]; st[3] = r.keys[1]; st[4] = r.rows.y0; st[5] = r.rows.y1;
    st[6] = r.early ? (int)(r.early - buf) : 0;
    return ret;
}

// A filter under the stripe [fy0, fy1), then maps from elsewhere that cover [cy0, cy1) (an upload, a gather, the SGM stage), then the
// select of the minima still pending: y = the rows the results cover after the foreign maps and after the select.
void rows_across_foreign_maps(int fy0, int fy1, int cy0, int cy1, int *y)
{
    Results r;
    filtered(r, Rows{fy0, fy1}, nullptr);
    cover(r, Rows{cy0, cy1});
    maps_written(r);
    y[0] = r.rows.y0; y[1] = r.rows.y1;
    cover_filtered(r);
    maps_written(r);
    y[2] = r.rows.y0; y[3] = r.rows.y1;
}

int rows_whole(int H, int y0, int y1) { return Rows{y0, y1} == whole_image(H); }

// One transition of the image pair's bookkeeping.  st = {depth, next depth, slot, range pending, inside} in and out; returns the
// slot (op 3), else the answers: bit 0 a pair is staged, from bit 1 on the depth at the next construct + 1.
int pair_step(int *st, int op, int a, int b)
{
    PairState p;
    p.depth = st[0]; p.next_depth = st[1]; p.slot = st[2]; p.range_pending = st[3] != 0; p.inside = st[4] != 0;
    int slot = -1;
    switch (op) {
    case 0: uploaded(p, a, b != 0); break;
    case 1: staged(p, a, b != 0); break;
    case 2: adopted(p, a != 0); break;
    case 3: slot = next_slot(p); break;
    case 4: staged(p, p.next_depth, false); break;       // its range has arrived
    case 5: p = PairState{}; break;       // a new record
    default: break;                       // (the questions of the state as it is)
    }
    st[0] = p.depth; st[1] = p.next_depth; st[2] = p.slot; st[3] = p.range_pending; st[4] = p.inside;
    return op == 3 ? slot : (int)pair_staged(p) | (depth_at_construct(p) + 1) << 1;
}

}  // extern "C"

#ifdef PROBE_MAIN
// The same records walked natively, for a build under -fsanitize=address,undefined (tests/test_ctx_state.py runs it): every move of
// every record from every state a short random walk reaches.  Prints the number of steps; a sanitizer report fails the run.
#include <cstdio>

int main()
{
    unsigned seed = 12345u, steps = 0;
    auto rnd = [&](unsigned n) { seed = seed * 1664525u + 1013904223u; return (int)((seed >> 8) % n); };
    int side[3] = {0, 0, 0}, res[7] = {0, 0, 0, 0, 0, 0, 0}, pair[5] = {-1, -1, 0, 0, 1}, y[4];
    for (int i = 0; i < 20000; ++i, steps += 3) {
        side_step(side, rnd(6), 2 << rnd(3));
        const int y0 = rnd(60), op = rnd(11);
        res_step(res, op, op == 8 ? rnd(2) : y0, y0 + 1 + rnd(60 - y0), rnd(3));
        pair_step(pair, rnd(7), rnd(2), rnd(2));
        if (pair[2] != 0 && pair[2] != 1) return 1;       // (the slot indexes two events and two halves of the staging memory)
    }
    rows_across_foreign_maps(20, 40, 0, 60, y);
    printf("%u steps, rows %d %d %d %d, whole %d\n", steps, y[0], y[1], y[2], y[3], rows_whole(60, 0, 60));
    return 0;
}
#endif
