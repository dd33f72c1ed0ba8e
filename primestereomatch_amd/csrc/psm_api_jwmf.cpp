// psm_api_jwmf.cpp - psm_joint_wmf: the joint weighted median of the reference's live PP::processDM (src/PP.cpp:402-424,
// include/JointWMF.h) on the device maps, behind the C ABI.  Kernels: psm_jwmf.hip.  Semantics: DESIGN.md section 9.
#include "psm_ctx.h"

#include <algorithm>
#include <cmath>

using namespace psm;

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
        if (!c->jw_user[s] && !(c->jw_have[s] && c->jw_params[s][0] == n_clusters && c->jw_params[s][1] == max_iter) &&
            kmeans(c, s, sc[s], n_clusters, max_iter)) return 1;
    // The integer weight table of a side is formed on the host (libm expf: the reference's float table) once per clustering
    // and sigma, into page-locked staging (a pageable source would make the copy wait for the stream to drain); the staging
    // of a side is refilled only after the copy out of it has executed.
    const size_t TAB = (size_t)JW_NF_MAX * JW_NF_MAX;
    for (int s = 0; s < 2; ++s) {
        if (c->jw_tab_ok[s] && c->jw_tab_sigma[s] == sigma) continue;
        if (!c->jw_pin) PSM_HIP(c, hipHostMalloc((void **)&c->jw_pin, 2 * TAB * sizeof(unsigned long long), hipHostMallocDefault));
        if (!c->ev_jw[s]) PSM_HIP(c, hipEventCreateWithFlags(&c->ev_jw[s], hipEventDisableTiming));
        else PSM_HIP(c, hipEventSynchronize(c->ev_jw[s]));
        unsigned long long *st = c->jw_pin + s * TAB;
        std::fill(st, st + TAB, 0ull);
        weight_table(c->jw_centres[s], c->jw_nf[s], sigma, st);
        PSM_HIP(c, hipMemcpyAsync(sc[s].wq, st, TAB * sizeof(unsigned long long), hipMemcpyHostToDevice, c->stream));
        PSM_HIP(c, hipEventRecord(c->ev_jw[s], c->stream));
        c->jw_tab_ok[s] = true;
        c->jw_tab_sigma[s] = sigma;
    }
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
