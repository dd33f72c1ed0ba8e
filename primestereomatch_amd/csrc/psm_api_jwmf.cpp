// psm_api_jwmf.cpp - psm_joint_wmf: the joint weighted median of the reference's live PP::processDM (src/PP.cpp:402-424,
// include/JointWMF.h) on the device maps, behind the C ABI.  Kernels: psm_jwmf.hip.  Semantics: DESIGN.md section 9.
// psm_joint_wmf_batch: the same for the maps of several contexts.  Both are one launch sequence (jw_enqueue): the images to cluster
// and the map sides lie on a grid axis, whether they are the two of one pair or those of many.
#include "psm_ctx.h"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace psm;

namespace psm {

void jwmf_batch_free(psm_ctx *c)
{
    JwBatch &b = c->jwb;
    table_free(b.tab);
    (void)hipFree(b.block); b.block = nullptr;
    if (b.pin) (void)hipHostFree(b.pin);
    b.pin = nullptr;
    b.cap = 0;
}

}  // namespace psm

namespace {

constexpr unsigned long long JW_SEED = 0x4A574D46ull;   // splitmix64 state of the k-means++ seeding (tests/jwmf_model.py SEED)
constexpr int JW_GROUP = 16;                            // Lloyd iterations launched between two looks at the convergence flags

// One side's part of the device block c->jw (every part 256-byte aligned), and the part's size
struct JwScratch {
    unsigned *bits, *samples, *kt, *d2t;
    int *labels, *sums;
    uint8_t *lok, *F, *out;
    unsigned long long *wq;
    size_t bytes;
};

// b == nullptr: only the size is wanted
JwScratch carve(uint8_t *b, size_t HW)
{
    JwScratch s;
    size_t off = 0;
    auto take = [&](size_t n) { uint8_t *p = b ? b + off : nullptr; off += (n + 255) / 256 * 256; return p; };
    s.bits = (unsigned *)take(JW_KEYS / 8);
    s.samples = (unsigned *)take((size_t)JW_KEYS * 4);
    s.kt = (unsigned *)take((size_t)JW_KEYS * 4);
    s.d2t = (unsigned *)take((size_t)JW_KEYS * 4);
    s.labels = (int *)take((size_t)JW_KEYS * 4);
    s.sums = (int *)take(JW_NF_MAX * 4 * 4);
    s.lok = take(JW_KEYS);
    s.wq = (unsigned long long *)take((size_t)JW_NF_MAX * JW_NF_MAX * 8);
    s.F = take(HW);
    s.out = take(HW);
    s.bytes = off;
    return s;
}

int ensure_jw(psm_ctx *c, JwScratch sc[2])
{
    const size_t HW = (size_t)c->W * c->H, per = carve(nullptr, HW).bytes;
    if (!c->jw) PSM_HIP(c, hipMalloc((void **)&c->jw, 2 * per));
    for (int s = 0; s < 2; ++s) sc[s] = carve(c->jw + s * per, HW);
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
// of a side is refilled only after the copy out of it has executed.  st: the stream the copies go on (the call's first
// context's); e: the context that receives an error message.
int upload_tables(psm_ctx *e, psm_ctx *c, const JwScratch sc[2], float sigma, hipStream_t st)
{
    const size_t TAB = (size_t)JW_NF_MAX * JW_NF_MAX;
    for (int s = 0; s < 2; ++s) {
        JwClust &cl = c->jw_cl[s];
        if (cl.tab_ok && cl.tab_sigma == sigma) continue;
        if (!c->jw_pin) PSM_HIP(e, hipHostMalloc((void **)&c->jw_pin, 2 * TAB * sizeof(unsigned long long), hipHostMallocDefault));
        if (!c->ev_jw[s]) PSM_HIP(e, hipEventCreateWithFlags(&c->ev_jw[s], hipEventDisableTiming));
        else PSM_HIP(e, hipEventSynchronize(c->ev_jw[s]));
        unsigned long long *pin = c->jw_pin + s * TAB;
        std::fill(pin, pin + TAB, 0ull);
        weight_table(cl.centres, cl.nf, sigma, pin);
        PSM_HIP(e, hipMemcpyAsync(sc[s].wq, pin, TAB * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
        PSM_HIP(e, hipEventRecord(c->ev_jw[s], st));
        cl.tab_ok = true;
        cl.tab_sigma = sigma;
    }
    return 0;
}

// The records of a call of several contexts as its device table holds them (c0->jwb.tab): the images to cluster in
// front, the 2 n map sides behind the room for 2 n images - an offset that is the call's, whatever m is
std::vector<uint8_t> table_records(const std::vector<JwImg> &img, const std::vector<JwSide> &sides)
{
    std::vector<uint8_t> recs(sides.size() * (sizeof(JwImg) + sizeof(JwSide)), 0);
    if (!img.empty()) memcpy(recs.data(), img.data(), img.size() * sizeof(JwImg));
    memcpy(recs.data() + sides.size() * sizeof(JwImg), sides.data(), sides.size() * sizeof(JwSide));
    return recs;
}

// The stage for the maps of the n contexts of one call: the only statement of its defaults, limits and preconditions,
// its launch order, Prof brackets, launch checks, the group loop and the adoption of the clusterings.  who: the entry's name in the
// messages; single: the entry is psm_joint_wmf.  The device k-means of a side runs once per pair and parameters - a clustering the
// host set, or one made by an earlier call with the same n_clusters / max_iter, is used as it is.  The chains of the m images that do
// need one run side by side: one seeding workgroup per image in one launch, every Lloyd iteration two launches for all of them,
// one look at all convergence flags per JW_GROUP iterations; the median runs as one grid over the 2 n map sides.  Buffers stay per
// context (JwScratch), but for Lloyd states and centres, which lie in a block of ctxs[0] (JwBatch).  With m == 0 nothing here
// synchronises with the host.  Every context of a batch ends where its own psm_joint_wmf(ctx, ..., NULL, NULL, 0) would have left it.
// What differs between a single call and a batch, and nothing else:
//   - n == 1 (either entry): the at most two JwImg / two JwSide records go to the kernels by value in the kernarg, so such a call
//     neither allocates nor uploads a device table; n > 1: the records are uploaded as ctxs[0]'s table (table_records);
//   - n > 1 only: the other contexts' streams are ordered before and behind the shared launches by events;
//   - psm_joint_wmf only: copy_maps_out behind this function, by the entry itself (which is why the closing synchronisation and
//     the stage time are the entries').
int jw_enqueue(const char *who, bool single, psm_ctx *const *ctxs, int n, int radius, float sigma, int n_clusters, int max_iter)
{
    psm_ctx *c0 = ctxs[0];
    if (radius <= 0) radius = 9;               // MED_SZ / 2 (include/PP.h:12, src/PP.cpp:421-422)
    if (!(sigma > 0.f)) sigma = 25.5f;         // JointWMF::filter's defaults (JointWMF.h:81)
    if (n_clusters <= 0) n_clusters = 256;
    if (max_iter <= 0) max_iter = 10000;       // TermCriteria(..., 10000) (JointWMF.h:590)
    if (radius > JW_RMAX) return fail(c0, "%s: radius %d outside 1..%d", who, radius, JW_RMAX);
    if (n_clusters > JW_NF_MAX) return fail(c0, "%s: n_clusters %d outside 1..%d", who, n_clusters, JW_NF_MAX);
    for (int i = 0; i < n; ++i) {
        if (batch_member(c0, who, ctxs, i)) return 1;
        psm_ctx *c = ctxs[i];
        const std::string at = single ? "this context" : "context " + std::to_string(i);
        if (c->W != c0->W || c->H != c0->H || c->device != c0->device)
            return fail(c0, "%s: %s has another width / height / device than context 0", who, at.c_str());
        if (!c->res.maps) return fail(c0, "%s: %s has no disparity maps", who, at.c_str());
        if (stripe_only(c)) return fail(c0, "%s: the maps of %s hold its row stripe only (gather the stripes first)", who, at.c_str());
        if (!c->have_images || c->pair.st.depth < 0) return fail(c0, "%s: %s has no image pair uploaded (the feature images)", who, at.c_str());
        if (c->pair.st.depth != c0->pair.st.depth) return fail(c0, "%s: %s holds images of another depth than context 0", who, at.c_str());
    }
    if (bind(c0)) return 1;
    hipStream_t s = c0->stream;
    JwBatch &t = c0->jwb;
    const bool table = n > 1;
    const size_t HW = (size_t)c0->W * c0->H, NS = 2 * (size_t)n;            // NS: map sides, and images at most
    const size_t CEN = (size_t)JW_NF_MAX * 3 * sizeof(float), ST = 4 * sizeof(int);
    const std::string stage = who + 4;                                      // (behind "psm_": as the launch checks name the stage)
    auto launched = [&](const char *what) { return check_launch(c0, (stage + " (" + what + ")").c_str()); };

    // ---- buffers, events, the block's and the table's memory: before any launch ----
    std::vector<JwScratch> sc(NS);
    for (int i = 0; i < n; ++i)
        if (ensure_jw(ctxs[i], &sc[2 * (size_t)i])) return member_failed(c0, who, i, ctxs[i]);
    if (batch_events(c0, ctxs, n)) return 1;
    if (t.cap < NS) {
        PSM_HIP(c0, hipStreamSynchronize(s));
        (void)hipFree(t.block);
        if (t.pin) (void)hipHostFree(t.pin);
        t.block = t.pin = nullptr;
        t.cap = 0;
        PSM_HIP(c0, hipMalloc((void **)&t.block, NS * (ST + CEN)));
        PSM_HIP(c0, hipHostMalloc((void **)&t.pin, NS * (ST + CEN), hipHostMallocDefault));
        t.cap = NS;
    }
    int *const st_dev = (int *)t.block, *const st_pin = (int *)t.pin;
    float *const cen_dev = (float *)(t.block + t.cap * ST), *const cen_pin = (float *)(t.pin + t.cap * ST);

    // ---- the records: the images to cluster (m <= 2 n), the 2 n map sides ----
    struct Member { psm_ctx *c; int side; };
    std::vector<Member> mem;
    std::vector<JwImg> img;
    std::vector<JwSide> sides;
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < 2; ++k) {
            psm_ctx *c = ctxs[i];
            const JwClust &cl = c->jw_cl[k];
            const JwScratch &q = sc[2 * (size_t)i + k];
            sides.push_back(JwSide{c->pair.raw[k], q.lok, q.F, c->maps + k * HW, q.wq, q.out});
            if (cl.user || (cl.have && cl.n_clusters == n_clusters && cl.max_iter == max_iter)) continue;
            const size_t j = mem.size();
            mem.push_back(Member{c, k});
            img.push_back(JwImg{c->pair.raw[k], q.bits, q.samples, q.kt, q.d2t, q.labels, q.sums, st_dev + 4 * j, cen_dev + j * JW_NF_MAX * 3, q.lok, 0, 0});
        }
    const int m = (int)mem.size();
    std::vector<uint8_t> recs;
    bool fresh = false;
    if (table) {
        recs = table_records(img, sides);
        if (table_reserve(c0, t.tab, recs.data(), recs.size(), &fresh)) return 1;
    }
    const JwRecs<JwImg> im{img.data(), table ? (const JwImg *)t.tab.dev : nullptr, m};
    const JwRecs<JwSide> sd{sides.data(), table ? (const JwSide *)(t.tab.dev + NS * sizeof(JwImg)) : nullptr, (int)NS};

    // ---- every context's earlier work (uploads, downloads of its maps, a call of its own) is ordered before the shared launches ----
    for (int i = 0; i < n; ++i)
        if (maps_writable(ctxs[i])) return member_failed(c0, who, i, ctxs[i]);
    if (batch_join(c0, ctxs, n)) return 1;
    if (fresh && table_upload(c0, t.tab, recs.data(), recs.size())) return 1;

    // ---- the default clustering of the m images (tests/jwmf_model.py cluster): keys, ordered samples, identity or k-means++ +
    // Lloyd; leaves label_of_key in the side's lok.  Synchronises with the host. ----
    if (m > 0) {
        for (const Member &e : mem) e.c->jw_cl[e.side].gone();                  // (their buffers are about to be rewritten)
        {
            Prof p(c0, PSM_K_JWMF);
            PSM_HIP(c0, hipMemsetAsync(st_dev, 0, (size_t)m * ST, s));
            launch_jw_keys(s, im, c0->pair.st.depth, HW);
            launch_jw_compact(s, im);
        }
        if (launched("keys")) return 1;
        PSM_HIP(c0, hipMemcpyAsync(st_pin, st_dev, (size_t)m * ST, hipMemcpyDeviceToHost, s));
        PSM_HIP(c0, hipStreamSynchronize(s));
        int n_all = 0, n_km = 0;              // the largest sample count of all images / of those that run the k-means
        bool any_id = false;
        for (int j = 0; j < m; ++j) {
            const int ns = st_pin[4 * j + 3];
            img[j].n = ns;
            img[j].nf = std::min(ns, n_clusters);
            n_all = std::max(n_all, ns);
            if (ns <= n_clusters) any_id = true;
            else n_km = std::max(n_km, ns);
        }
        if (table) {                            // (n, nf; by value they are the next launch's argument)
            recs = table_records(img, sides);
            if (table_upload(c0, t.tab, recs.data(), recs.size())) return 1;
        }
        {
            Prof p(c0, PSM_K_JWMF);
            if (any_id) launch_jw_identity(s, im, n_clusters);
            if (n_km) launch_jw_seed(s, im, n_clusters, JW_SEED);
        }
        if (launched("seeding")) return 1;
        // An image that has converged (or is its own clustering) does nothing in the iterations that follow: its flag freezes it
        // while the others go on.  One look at all flags per group.
        bool all = n_km == 0;
        for (int it = 0; it < max_iter && !all;) {
            const int g = std::min(max_iter - it, JW_GROUP);
            {
                Prof p(c0, PSM_K_JWMF);
                for (int k = 0; k < g; ++k) launch_jw_lloyd(s, im, n_km, it + k);
            }
            if (launched("k-means")) return 1;
            it += g;
            PSM_HIP(c0, hipMemcpyAsync(st_pin, st_dev, (size_t)m * ST, hipMemcpyDeviceToHost, s));
            PSM_HIP(c0, hipStreamSynchronize(s));
            all = true;
            for (int j = 0; j < m; ++j) all = all && st_pin[4 * j + 1] != 0;
        }
        {
            Prof p(c0, PSM_K_JWMF);
            launch_jw_lok(s, im, n_all);
        }
        if (launched("clusters")) return 1;
        PSM_HIP(c0, hipMemcpyAsync(cen_pin, cen_dev, (size_t)m * CEN, hipMemcpyDeviceToHost, s));
        PSM_HIP(c0, hipStreamSynchronize(s));
        for (int j = 0; j < m; ++j) {
            const int iters = img[j].n <= n_clusters ? 0 : (st_pin[4 * j + 1] ? st_pin[4 * j + 2] : max_iter);
            mem[j].c->jw_cl[mem[j].side].adopted(img[j].nf, iters, n_clusters, max_iter, cen_pin + (size_t)j * JW_NF_MAX * 3);
        }
    }

    // ---- weight tables (each through its own context's staging), cluster planes, the median, out -> maps ----
    for (int i = 0; i < n; ++i)
        if (upload_tables(c0, ctxs[i], &sc[2 * (size_t)i], sigma, s)) return 1;
    {
        Prof p(c0, PSM_K_JWMF);
        launch_jw_plane(s, sd, c0->pair.st.depth, HW);
        launch_jw_median(s, sd, c0->W, c0->H, radius);
    }
    if (launched("median")) return 1;
    // (the feature images are the image slots: the keys and the cluster planes are formed from them, the median reads the planes)
    for (int i = 0; i < n; ++i)
        if (images_read(ctxs[i], s)) return member_failed(c0, who, i, ctxs[i]);
    for (size_t q = 0; q < NS; ++q)
        PSM_HIP(c0, hipMemcpyAsync(ctxs[q / 2]->maps + (q & 1) * HW, sc[q].out, HW, hipMemcpyDeviceToDevice, s));
    for (int i = 0; i < n; ++i) forget_early(ctxs[i]->res);        // (rewritten in place)
    return batch_fork(c0, ctxs, n);
}

}  // namespace

extern "C" {

int psm_joint_wmf(psm_ctx *c, int radius, float sigma, int n_clusters, int max_iter, uint8_t *lmap, uint8_t *rmap, size_t stride)
{
    if (!c) return 1;
    const double t0 = now_us();
    if (jw_enqueue("psm_joint_wmf", true, &c, 1, radius, sigma, n_clusters, max_iter)) return 1;
    if (copy_maps_out(c, c->maps, lmap, rmap, stride)) return 1;
    if (!c->opt_async) PSM_HIP(c, hipStreamSynchronize(c->stream));
    c->stage_us[PSM_STAGE_PP] += now_us() - t0;
    return 0;
}

int psm_joint_wmf_batch(psm_ctx *const *ctxs, int n, int radius, float sigma, int n_clusters, int max_iter)
{
    const char *who = "psm_joint_wmf_batch";
    if (!ctxs || n < 1 || !ctxs[0]) return fail(nullptr, "%s: bad arguments", who);
    psm_ctx *c0 = ctxs[0];
    if (n > 4096) return fail(c0, "%s: %d pairs (at most 4096 per call)", who, n);
    const double t0 = now_us();
    if (jw_enqueue(who, false, ctxs, n, radius, sigma, n_clusters, max_iter)) return 1;
    if (!c0->opt_async) PSM_HIP(c0, hipStreamSynchronize(c0->stream));
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
    c->jw_cl[side].gone();                            // (its lok is about to be rewritten)
    PSM_HIP(c, hipMemcpyAsync(sc[side].lok, label_of_key, JW_KEYS, hipMemcpyHostToDevice, c->stream));
    PSM_HIP(c, hipStreamSynchronize(c->stream));      // (the caller's buffer is free again)
    c->jw_cl[side].set_by_host(n_clusters, centres);
    return 0;
}

int psm_joint_wmf_clusters(psm_ctx *c, int side, int *n_clusters, float *centres, uint8_t *label_of_key, int *iterations)
{
    if (!c) return 1;
    if (side != PSM_LEFT && side != PSM_RIGHT) return fail(c, "psm_joint_wmf_clusters: bad side %d", side);
    const JwClust &cl = c->jw_cl[side];
    if (!cl.have) return fail(c, "psm_joint_wmf_clusters: no clustering for this side of the current pair");
    if (n_clusters) *n_clusters = cl.nf;
    if (iterations) *iterations = cl.iters;
    if (centres) std::copy(cl.centres.begin(), cl.centres.end(), centres);
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
