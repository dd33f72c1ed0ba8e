// psm_api_jwmf.cpp - psm_joint_wmf: the joint weighted median of the reference's live PP::processDM (src/PP.cpp:402-424,
// include/JointWMF.h) on the device maps, behind the C ABI.  Kernels: psm_jwmf.hip.  Semantics: DESIGN.md section 9.
// psm_joint_wmf_batch: the same for the maps of several contexts in shared launches, the image or map side on a grid axis.
#include "psm_ctx.h"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace psm;

namespace psm {

void jwmf_batch_free(psm_ctx *c)
{
    JwBatch &b = c->jwb;
    (void)hipFree(b.tab); b.tab = nullptr;
    if (b.tab_pin) (void)hipHostFree(b.tab_pin);
    b.tab_pin = nullptr;
    b.tab_cap = 0;
    b.tab_host.clear();
    for (hipEvent_t &e : b.ev_tab) { if (e) (void)hipEventDestroy(e); e = nullptr; }
    (void)hipFree(b.block); b.block = nullptr;
    if (b.pin) (void)hipHostFree(b.pin);
    b.pin = nullptr;
    b.cap = 0;
}

}  // namespace psm

namespace {

constexpr unsigned long long JW_SEED = 0x4A574D46ull;   // splitmix64 state of the k-means++ seeding (tests/jwmf_model.py SEED)
constexpr int JW_GROUP = 16;                            // Lloyd iterations launched between two looks at the convergence flag

// One side's part of the device block c->jw (offsets in bytes, every part 256-byte aligned)
struct JwScratch {
    unsigned *bits, *samples, *kt, *d2t;
    int *labels, *sums, *state;            // state: {changed, converged, iterations, sample count}
    float *centres;
    uint8_t *lok, *F, *out;
    unsigned long long *wq;
};

size_t al(size_t b) { return (b + 255) / 256 * 256; }

size_t side_bytes(size_t HW)
{
    return al(JW_KEYS / 8) + 4 * al((size_t)JW_KEYS * 4) + al(JW_NF_MAX * 4 * 4) + al(16 * 4) + al(JW_NF_MAX * 3 * 4) +
           al(JW_KEYS) + al((size_t)JW_NF_MAX * JW_NF_MAX * 8) + 2 * al(HW);
}

JwScratch carve(uint8_t *b, size_t HW)
{
    JwScratch s;
    auto take = [&](size_t n) { uint8_t *p = b; b += al(n); return p; };
    s.bits = (unsigned *)take(JW_KEYS / 8);
    s.samples = (unsigned *)take((size_t)JW_KEYS * 4);
    s.kt = (unsigned *)take((size_t)JW_KEYS * 4);
    s.d2t = (unsigned *)take((size_t)JW_KEYS * 4);
    s.labels = (int *)take((size_t)JW_KEYS * 4);
    s.sums = (int *)take(JW_NF_MAX * 4 * 4);
    s.state = (int *)take(16 * 4);
    s.centres = (float *)take(JW_NF_MAX * 3 * 4);
    s.lok = take(JW_KEYS);
    s.wq = (unsigned long long *)take((size_t)JW_NF_MAX * JW_NF_MAX * 8);
    s.F = take(HW);
    s.out = take(HW);
    return s;
}

int ensure_jw(psm_ctx *c, JwScratch sc[2])
{
    const size_t HW = (size_t)c->W * c->H, per = side_bytes(HW);
    if (!c->jw) PSM_HIP(c, hipMalloc((void **)&c->jw, 2 * per));
    for (int s = 0; s < 2; ++s) sc[s] = carve(c->jw + s * per, HW);
    return 0;
}

// The default clustering of one side on the device (tests/jwmf_model.py cluster): keys, ordered samples, identity or
// k-means++ + Lloyd; leaves label_of_key in sc.lok and the centres in c->jw_centres[side].  Synchronises with the host.
int kmeans(psm_ctx *c, int side, const JwScratch &sc, int n_clusters, int max_iter)
{
    const size_t HW = (size_t)c->W * c->H;
    int n = 0;
    {
        Prof p(c, PSM_K_JWMF);
        PSM_HIP(c, hipMemsetAsync(sc.bits, 0, JW_KEYS / 8, c->stream));
        launch_jw_keys(c->stream, c->raw[side], c->raw_depth, HW, sc.bits);
        launch_jw_compact(c->stream, sc.bits, sc.samples, sc.state + 3);
    }
    if (check_launch(c, "joint_wmf (keys)")) return 1;
    PSM_HIP(c, hipMemcpyAsync(&n, sc.state + 3, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    PSM_HIP(c, hipStreamSynchronize(c->stream));
    const int nf = n < n_clusters ? n : n_clusters;
    int iters = 0;
    if (n <= n_clusters) {
        Prof p(c, PSM_K_JWMF);
        launch_jw_identity(c->stream, sc.samples, n, sc.centres, sc.labels);
    } else {
        {
            Prof p(c, PSM_K_JWMF);
            launch_jw_seed(c->stream, sc.samples, n, nf, JW_SEED, sc.centres, sc.kt, sc.d2t);
            PSM_HIP(c, hipMemsetAsync(sc.labels, 0xff, (size_t)n * 4, c->stream));     // (-1: the first assignment changes every label)
            PSM_HIP(c, hipMemsetAsync(sc.sums, 0, JW_NF_MAX * 4 * 4, c->stream));
            PSM_HIP(c, hipMemsetAsync(sc.state, 0, 3 * sizeof(int), c->stream));
        }
        int st[3] = {0, 0, 0};
        // Iterations after convergence return at once (the device flag), so the host looks at the flag once per group
        for (int it = 0; it < max_iter && !st[1];) {
            const int g = max_iter - it < JW_GROUP ? max_iter - it : JW_GROUP;
            {
                Prof p(c, PSM_K_JWMF);
                for (int k = 0; k < g; ++k) launch_jw_lloyd(c->stream, sc.samples, n, nf, sc.centres, sc.labels, sc.sums, sc.state, it + k);
            }
            if (check_launch(c, "joint_wmf (k-means)")) return 1;
            it += g;
            PSM_HIP(c, hipMemcpyAsync(st, sc.state, sizeof(st), hipMemcpyDeviceToHost, c->stream));
            PSM_HIP(c, hipStreamSynchronize(c->stream));
        }
        iters = st[1] ? st[2] : max_iter;
    }
    {
        Prof p(c, PSM_K_JWMF);
        PSM_HIP(c, hipMemsetAsync(sc.lok, 0, JW_KEYS, c->stream));
        launch_jw_lok(c->stream, sc.samples, n, sc.labels, sc.lok);
    }
    if (check_launch(c, "joint_wmf (clusters)")) return 1;
    c->jw_centres[side].resize((size_t)nf * 3);
    PSM_HIP(c, hipMemcpyAsync(c->jw_centres[side].data(), sc.centres, (size_t)nf * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    PSM_HIP(c, hipStreamSynchronize(c->stream));
    c->jw_nf[side] = nf;
    c->jw_iters[side] = iters;
    c->jw_params[side][0] = n_clusters;
    c->jw_params[side][1] = max_iter;
    c->jw_have[side] = true;
    c->jw_tab_ok[side] = false;
    return 0;
}

// The weight table of JointWMF.h:615-645 ("exp") over the centres, with the host's libm expf (the reference's own
// function: a float argument under `using namespace std`), as the exact integers rint(w * 2^48).
void weight_table(const std::vector<float> &cen, int nf, float sigma, unsigned long long *wq)
{
    const float nSigmaI = sigma / 256.0f * 64;
    const float divider = 1.0f / (2 * nSigmaI * nSigmaI);
    for (int i = 0; i < nf; ++i)
        for (int j = i; j < nf; ++j) {
            const float d0 = cen[3 * i] - cen[3 * j], d1 = cen[3 * i + 1] - cen[3 * j + 1], d2 = cen[3 * i + 2] - cen[3 * j + 2];
            const float s = d0 * d0 + d1 * d1 + d2 * d2;
            const float w = expf(-s * divider);
            const unsigned long long q = (unsigned long long)std::nearbyint((double)w * 281474976710656.0);   // 2^48: exact
            wq[(size_t)i * JW_NF_MAX + j] = wq[(size_t)j * JW_NF_MAX + i] = q;
        }
}

// The integer weight table of a side is formed on the host (libm expf: the reference's float table) once per clustering
// and sigma, into page-locked staging (a pageable source would make the copy wait for the stream to drain); the staging
// of a side is refilled only after the copy out of it has executed.  st: the stream the copies go on (a batch: its first
// context's); e: the context that receives an error message.
int upload_tables(psm_ctx *e, psm_ctx *c, const JwScratch sc[2], float sigma, hipStream_t st)
{
    const size_t TAB = (size_t)JW_NF_MAX * JW_NF_MAX;
    for (int s = 0; s < 2; ++s) {
        if (c->jw_tab_ok[s] && c->jw_tab_sigma[s] == sigma) continue;
        if (!c->jw_pin) PSM_HIP(e, hipHostMalloc((void **)&c->jw_pin, 2 * TAB * sizeof(unsigned long long), hipHostMallocDefault));
        if (!c->ev_jw[s]) PSM_HIP(e, hipEventCreateWithFlags(&c->ev_jw[s], hipEventDisableTiming));
        else PSM_HIP(e, hipEventSynchronize(c->ev_jw[s]));
        unsigned long long *pin = c->jw_pin + s * TAB;
        std::fill(pin, pin + TAB, 0ull);
        weight_table(c->jw_centres[s], c->jw_nf[s], sigma, pin);
        PSM_HIP(e, hipMemcpyAsync(sc[s].wq, pin, TAB * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
        PSM_HIP(e, hipEventRecord(c->ev_jw[s], st));
        c->jw_tab_ok[s] = true;
        c->jw_tab_sigma[s] = sigma;
    }
    return 0;
}

// a side takes part in the device k-means unless the host set its clustering or an earlier call made it with these parameters
bool needs_kmeans(const psm_ctx *c, int s, int n_clusters, int max_iter)
{
    return !c->jw_user[s] && !(c->jw_have[s] && c->jw_params[s][0] == n_clusters && c->jw_params[s][1] == max_iter);
}

// psm_joint_wmf_batch: the batch's device table to the device if it differs from the one there (t.tab_host), through one of two
// page-locked slots - the copy is stream-ordered behind the kernels that still read the old table, and a slot is rewritten only
// after the copy that read it has executed
int upload_batch_table(psm_ctx *c0, const std::vector<uint8_t> &tab)
{
    JwBatch &t = c0->jwb;
    if (t.tab_host == tab) return 0;
    const int slot = t.tab_slot ^= 1;
    PSM_HIP(c0, hipEventSynchronize(t.ev_tab[slot]));
    uint8_t *pin = t.tab_pin + (size_t)slot * t.tab_cap;
    memcpy(pin, tab.data(), tab.size());
    t.tab_host = tab;
    PSM_HIP(c0, hipMemcpyAsync(t.tab, pin, tab.size(), hipMemcpyHostToDevice, c0->stream));
    PSM_HIP(c0, hipEventRecord(t.ev_tab[slot], c0->stream));
    return 0;
}

}  // namespace

extern "C" {

int psm_joint_wmf(psm_ctx *c, int radius, float sigma, int n_clusters, int max_iter, uint8_t *lmap, uint8_t *rmap, size_t stride)
{
    if (!c) return 1;
    if (radius <= 0) radius = 9;               // MED_SZ / 2 (include/PP.h:12, src/PP.cpp:421-422)
    if (!(sigma > 0.f)) sigma = 25.5f;         // JointWMF::filter's defaults (JointWMF.h:81)
    if (n_clusters <= 0) n_clusters = 256;
    if (max_iter <= 0) max_iter = 10000;       // TermCriteria(..., 10000) (JointWMF.h:590)
    if (radius > JW_RMAX) return fail(c, "psm_joint_wmf: radius %d outside 1..%d", radius, JW_RMAX);
    if (n_clusters > JW_NF_MAX) return fail(c, "psm_joint_wmf: n_clusters %d outside 1..%d", n_clusters, JW_NF_MAX);
    if (!c->res.maps) return fail(c, "psm_joint_wmf: no disparity maps computed");
    if (stripe_only(c)) return fail(c, "psm_joint_wmf: the maps hold this context's row stripe only (gather the stripes first)");
    if (!c->have_images) return fail(c, "psm_joint_wmf: no image pair uploaded (the feature images)");
    if (bind(c) || maps_writable(c)) return 1;
    const double t0 = now_us();
    JwScratch sc[2];
    if (ensure_jw(c, sc)) return 1;
    // the device k-means of a side runs once per pair and parameters: a clustering the host set, or one made by an earlier
    // call with the same n_clusters / max_iter, is used as it is
    for (int s = 0; s < 2; ++s)
        if (needs_kmeans(c, s, n_clusters, max_iter) && kmeans(c, s, sc[s], n_clusters, max_iter)) return 1;
    if (upload_tables(c, c, sc, sigma, c->stream)) return 1;
    const size_t HW = (size_t)c->W * c->H;
    JwPair pr;
    for (int s = 0; s < 2; ++s)
        pr.s[s] = JwSide{c->raw[s], sc[s].lok, sc[s].F, c->maps + s * HW, sc[s].wq, sc[s].out};
    {
        Prof p(c, PSM_K_JWMF);
        launch_jw_plane(c->stream, pr, c->raw_depth, HW);
        launch_jw_median(c->stream, pr, c->W, c->H, radius);
    }
    if (check_launch(c, "joint_wmf (median)")) return 1;
    for (int s = 0; s < 2; ++s)
        PSM_HIP(c, hipMemcpyAsync(c->maps + s * HW, sc[s].out, HW, hipMemcpyDeviceToDevice, c->stream));
    forget_early(c->res);        // (rewritten in place)
    if (copy_maps_out(c, c->maps, lmap, rmap, stride)) return 1;
    if (!c->opt_async) PSM_HIP(c, hipStreamSynchronize(c->stream));
    c->stage_us[PSM_STAGE_PP] += now_us() - t0;
    return 0;
}

// psm_joint_wmf of several contexts in shared launches ("several pairs per launch"): the clustering chains of the m
// images that need one run side by side - one seeding workgroup per image in one launch, every Lloyd iteration two launches for
// all of them, one look at all convergence flags per JW_GROUP iterations - and the median runs as one grid over the 2 n map sides.
// Buffers stay per context (JwScratch); the kernels reach them through a device table ctxs[0] owns.  Every context ends where its
// own psm_joint_wmf(ctx, ..., NULL, NULL, 0) would have left it.
int psm_joint_wmf_batch(psm_ctx *const *ctxs, int n, int radius, float sigma, int n_clusters, int max_iter)
{
    const char *who = "psm_joint_wmf_batch";
    if (!ctxs || n < 1 || !ctxs[0]) return fail(nullptr, "%s: bad arguments", who);
    psm_ctx *c0 = ctxs[0];
    if (n > 4096) return fail(c0, "%s: %d pairs (at most 4096 per call)", who, n);
    if (radius <= 0) radius = 9;               // (the defaults of psm_joint_wmf)
    if (!(sigma > 0.f)) sigma = 25.5f;
    if (n_clusters <= 0) n_clusters = 256;
    if (max_iter <= 0) max_iter = 10000;
    if (radius > JW_RMAX) return fail(c0, "%s: radius %d outside 1..%d", who, radius, JW_RMAX);
    if (n_clusters > JW_NF_MAX) return fail(c0, "%s: n_clusters %d outside 1..%d", who, n_clusters, JW_NF_MAX);
    for (int i = 0; i < n; ++i) {
        psm_ctx *c = ctxs[i];
        if (!c) return fail(c0, "%s: context %d is NULL", who, i);
        for (int j = 0; j < i; ++j)
            if (ctxs[j] == c) return fail(c0, "%s: context %d appears twice", who, i);
        if (c->W != c0->W || c->H != c0->H || c->device != c0->device)
            return fail(c0, "%s: context %d has another width / height / device than context 0", who, i);
        if (!c->res.maps) return fail(c0, "%s: context %d has no disparity maps", who, i);
        if (stripe_only(c)) return fail(c0, "%s: the maps of context %d hold its row stripe only (gather the stripes first)", who, i);
        if (!c->have_images || c->raw_depth < 0) return fail(c0, "%s: context %d has no image pair uploaded (the feature images)", who, i);
        if (c->raw_depth != c0->raw_depth) return fail(c0, "%s: context %d holds images of another depth than context 0", who, i);
    }
    if (bind(c0)) return 1;
    const double t0 = now_us();
    hipStream_t s = c0->stream;
    JwBatch &t = c0->jwb;
    const size_t HW = (size_t)c0->W * c0->H, NS = 2 * (size_t)n;            // NS: map sides, and images at most
    const size_t CEN = (size_t)JW_NF_MAX * 3 * sizeof(float), ST = 4 * sizeof(int);

    // ---- buffers, events and the table's memory: before any launch ----
    std::vector<JwScratch> sc(NS);
    for (int i = 0; i < n; ++i) {
        psm_ctx *c = ctxs[i];
        if (ensure_jw(c, &sc[2 * (size_t)i])) return c == c0 ? 1 : fail(c0, "%s: context %d: %s", who, i, c->err.c_str());
        if (c->stream != s && !c->ev_batch) PSM_HIP(c0, hipEventCreateWithFlags(&c->ev_batch, hipEventDisableTiming));
    }
    if (!c0->ev_batch) PSM_HIP(c0, hipEventCreateWithFlags(&c0->ev_batch, hipEventDisableTiming));
    const size_t tab_bytes = NS * (sizeof(JwImg) + sizeof(JwSide));
    if (t.tab_cap < tab_bytes || t.cap < NS) {
        PSM_HIP(c0, hipStreamSynchronize(s));
        jwmf_batch_free(c0);                 // (should an allocation below fail, the next call must not take the old table for current)
        PSM_HIP(c0, hipMalloc((void **)&t.tab, tab_bytes));
        PSM_HIP(c0, hipHostMalloc((void **)&t.tab_pin, 2 * tab_bytes, hipHostMallocDefault));
        PSM_HIP(c0, hipMalloc((void **)&t.block, NS * (ST + CEN)));
        PSM_HIP(c0, hipHostMalloc((void **)&t.pin, NS * (ST + CEN), hipHostMallocDefault));
        t.tab_cap = tab_bytes;
        t.cap = NS;
    }
    for (hipEvent_t &e : t.ev_tab)
        if (!e) PSM_HIP(c0, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    int *const st_dev = (int *)t.block, *const st_pin = (int *)t.pin;
    float *const cen_dev = (float *)(t.block + t.cap * ST), *const cen_pin = (float *)(t.pin + t.cap * ST);

    // ---- the table: the images to cluster (m <= 2 n) in front, the 2 n map sides from a fixed offset ----
    struct Member { int ctx, side; };
    std::vector<Member> mem;
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < 2; ++k)
            if (needs_kmeans(ctxs[i], k, n_clusters, max_iter)) mem.push_back(Member{i, k});
    const int m = (int)mem.size();
    std::vector<uint8_t> tab(t.tab_cap, 0);              // (the capacity's bytes: the sides' offset does not move with n)
    JwImg *const img = (JwImg *)tab.data();
    JwSide *const sides = (JwSide *)(tab.data() + t.cap * sizeof(JwImg));
    const JwImg *const img_dev = (const JwImg *)t.tab;
    const JwSide *const sides_dev = (const JwSide *)(t.tab + t.cap * sizeof(JwImg));
    for (int j = 0; j < m; ++j) {
        const psm_ctx *c = ctxs[mem[j].ctx];
        const JwScratch &q = sc[2 * (size_t)mem[j].ctx + mem[j].side];
        img[j] = JwImg{c->raw[mem[j].side], q.bits, q.samples, q.kt, q.d2t, q.labels, q.sums, st_dev + 4 * (size_t)j,
                       cen_dev + (size_t)j * JW_NF_MAX * 3, q.lok, 0, 0};
    }
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < 2; ++k) {
            const psm_ctx *c = ctxs[i];
            const JwScratch &q = sc[2 * (size_t)i + k];
            sides[2 * (size_t)i + k] = JwSide{c->raw[k], q.lok, q.F, c->maps + k * HW, q.wq, q.out};
        }

    // ---- every context's earlier work (uploads, downloads of its maps, a single call) is ordered before the shared launches ----
    for (int i = 0; i < n; ++i) {
        psm_ctx *c = ctxs[i];
        if (maps_writable(c)) return c == c0 ? 1 : fail(c0, "%s: context %d: %s", who, i, c->err.c_str());
        if (c->stream == s) continue;
        PSM_HIP(c0, hipEventRecord(c->ev_batch, c->stream));
        PSM_HIP(c0, hipStreamWaitEvent(s, c->ev_batch, 0));
    }
    if (upload_batch_table(c0, tab)) return 1;

    // ---- the default clustering of the m images (kmeans above, side by side); synchronises with the host ----
    if (m > 0) {
        for (const Member &e : mem) ctxs[e.ctx]->jw_have[e.side] = false;       // (their buffers are about to be rewritten)
        {
            Prof p(c0, PSM_K_JWMF);
            PSM_HIP(c0, hipMemsetAsync(st_dev, 0, (size_t)m * ST, s));
            launch_jw_keys_b(s, img_dev, m, c0->raw_depth, HW);
            launch_jw_compact_b(s, img_dev, m);
        }
        if (check_launch(c0, "joint_wmf_batch (keys)")) return 1;
        PSM_HIP(c0, hipMemcpyAsync(st_pin, st_dev, (size_t)m * ST, hipMemcpyDeviceToHost, s));
        PSM_HIP(c0, hipStreamSynchronize(s));
        int n_all = 0, n_km = 0;              // the largest sample count of all images / of those that run the k-means
        bool any_id = false;
        for (int j = 0; j < m; ++j) {
            const int ns = st_pin[4 * j + 3];
            img[j].n = ns;
            img[j].nf = ns < n_clusters ? ns : n_clusters;
            n_all = std::max(n_all, ns);
            if (ns <= n_clusters) any_id = true;
            else n_km = std::max(n_km, ns);
        }
        if (upload_batch_table(c0, tab)) return 1;
        {
            Prof p(c0, PSM_K_JWMF);
            if (any_id) launch_jw_identity_b(s, img_dev, m, n_clusters);
            if (n_km) launch_jw_seed_b(s, img_dev, m, n_clusters, JW_SEED);
        }
        if (check_launch(c0, "joint_wmf_batch (seeding)")) return 1;
        // An image that has converged (or is its own clustering) does nothing in the iterations that follow: its flag freezes it
        // while the others go on.  One look at all flags per group.
        bool all = n_km == 0;
        for (int it = 0; it < max_iter && !all;) {
            const int g = max_iter - it < JW_GROUP ? max_iter - it : JW_GROUP;
            {
                Prof p(c0, PSM_K_JWMF);
                for (int k = 0; k < g; ++k) launch_jw_lloyd_b(s, img_dev, m, n_km, it + k);
            }
            if (check_launch(c0, "joint_wmf_batch (k-means)")) return 1;
            it += g;
            PSM_HIP(c0, hipMemcpyAsync(st_pin, st_dev, (size_t)m * ST, hipMemcpyDeviceToHost, s));
            PSM_HIP(c0, hipStreamSynchronize(s));
            all = true;
            for (int j = 0; j < m; ++j) all = all && st_pin[4 * j + 1] != 0;
        }
        {
            Prof p(c0, PSM_K_JWMF);
            launch_jw_lok_b(s, img_dev, m, n_all);
        }
        if (check_launch(c0, "joint_wmf_batch (clusters)")) return 1;
        PSM_HIP(c0, hipMemcpyAsync(cen_pin, cen_dev, (size_t)m * CEN, hipMemcpyDeviceToHost, s));
        PSM_HIP(c0, hipStreamSynchronize(s));
        for (int j = 0; j < m; ++j) {
            psm_ctx *c = ctxs[mem[j].ctx];
            const int k = mem[j].side, nf = img[j].nf;
            const float *cen = cen_pin + (size_t)j * JW_NF_MAX * 3;
            c->jw_centres[k].assign(cen, cen + (size_t)nf * 3);
            c->jw_nf[k] = nf;
            c->jw_iters[k] = img[j].n <= n_clusters ? 0 : (st_pin[4 * j + 1] ? st_pin[4 * j + 2] : max_iter);
            c->jw_params[k][0] = n_clusters;
            c->jw_params[k][1] = max_iter;
            c->jw_have[k] = true;
            c->jw_tab_ok[k] = false;
        }
    }

    // ---- weight tables (each through its own context's staging), cluster planes, the median, out -> maps ----
    for (int i = 0; i < n; ++i)
        if (upload_tables(c0, ctxs[i], &sc[2 * (size_t)i], sigma, s)) return 1;
    {
        Prof p(c0, PSM_K_JWMF);
        launch_jw_plane_b(s, sides_dev, (int)NS, c0->raw_depth, HW);
        launch_jw_median_b(s, sides_dev, (int)NS, c0->W, c0->H, radius);
    }
    if (check_launch(c0, "joint_wmf_batch (median)")) return 1;
    for (size_t q = 0; q < NS; ++q)
        PSM_HIP(c0, hipMemcpyAsync(ctxs[q / 2]->maps + (q & 1) * HW, sc[q].out, HW, hipMemcpyDeviceToDevice, s));
    PSM_HIP(c0, hipEventRecord(c0->ev_batch, s));
    for (int i = 0; i < n; ++i) {
        psm_ctx *c = ctxs[i];
        forget_early(c->res);        // (rewritten in place)
        if (c->stream != s) PSM_HIP(c0, hipStreamWaitEvent(c->stream, c0->ev_batch, 0));
    }
    if (!c0->opt_async) PSM_HIP(c0, hipStreamSynchronize(s));
    const double dt = now_us() - t0;
    for (int i = 0; i < n; ++i) ctxs[i]->stage_us[PSM_STAGE_PP] += dt;
    return 0;
}

int psm_joint_wmf_set_clusters(psm_ctx *c, int side, int n_clusters, const float *centres, const uint8_t *label_of_key)
{
    if (!c) return 1;
    if (side != PSM_LEFT && side != PSM_RIGHT) return fail(c, "psm_joint_wmf_set_clusters: bad side %d", side);
    if (n_clusters < 1 || n_clusters > JW_NF_MAX) return fail(c, "psm_joint_wmf_set_clusters: n_clusters %d outside 1..%d", n_clusters, JW_NF_MAX);
    if (!centres || !label_of_key) return fail(c, "psm_joint_wmf_set_clusters: NULL centres or label_of_key");
    if (!c->have_images) return fail(c, "psm_joint_wmf_set_clusters: no image pair uploaded (clusters hold for the current pair)");
    for (int k = 0; k < JW_KEYS; ++k)
        if (label_of_key[k] >= n_clusters) return fail(c, "psm_joint_wmf_set_clusters: label_of_key[%d] = %d >= n_clusters %d", k, label_of_key[k], n_clusters);
    for (int i = 0; i < 3 * n_clusters; ++i)
        if (!std::isfinite(centres[i])) return fail(c, "psm_joint_wmf_set_clusters: centre component %d is not finite", i);
    if (bind(c)) return 1;
    JwScratch sc[2];
    if (ensure_jw(c, sc)) return 1;
    PSM_HIP(c, hipMemcpyAsync(sc[side].lok, label_of_key, JW_KEYS, hipMemcpyHostToDevice, c->stream));
    PSM_HIP(c, hipStreamSynchronize(c->stream));      // (the caller's buffer is free again)
    c->jw_centres[side].assign(centres, centres + 3 * n_clusters);
    c->jw_nf[side] = n_clusters;
    c->jw_iters[side] = 0;
    c->jw_have[side] = c->jw_user[side] = true;
    c->jw_tab_ok[side] = false;
    return 0;
}

int psm_joint_wmf_clusters(psm_ctx *c, int side, int *n_clusters, float *centres, uint8_t *label_of_key, int *iterations)
{
    if (!c) return 1;
    if (side != PSM_LEFT && side != PSM_RIGHT) return fail(c, "psm_joint_wmf_clusters: bad side %d", side);
    if (!c->jw_have[side]) return fail(c, "psm_joint_wmf_clusters: no clustering for this side of the current pair");
    if (n_clusters) *n_clusters = c->jw_nf[side];
    if (iterations) *iterations = c->jw_iters[side];
    if (centres) std::copy(c->jw_centres[side].begin(), c->jw_centres[side].end(), centres);
    if (label_of_key) {
        if (bind(c)) return 1;
        JwScratch sc[2];
        if (ensure_jw(c, sc)) return 1;
        PSM_HIP(c, hipMemcpyAsync(label_of_key, sc[side].lok, JW_KEYS, hipMemcpyDeviceToHost, c->stream));
        PSM_HIP(c, hipStreamSynchronize(c->stream));
    }
    return 0;
}

}  // extern "C"
