/* jwmf_reading.c - test-only: a serial restatement of the reference's JointWMF (include/JointWMF.h) as
 * PP::processDM calls it (src/PP.cpp:417-422), op for op where the result can depend on it: the column scan of
 * filterCore (JointWMF.h:173-410) with its joint histogram, its "necklace" lists of non-empty cells, the float
 * balanceWeight and its walk of the cut point; and, for images with at most nF distinct 6-bit keys (where every
 * clustering is the identity), featureIndexing's keys and weight table (JointWMF.h:546-645).
 * Built by tests/test_jwmf_model.py with cc -O2 -ffp-contract=off and loaded with ctypes.  Not product code: the
 * library computes the median from its definition. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

/* one cell count of a necklace-listed array: link i in when it becomes non-empty, unlink it when it becomes empty
 * (index 0 is the list head and is never linked) - JointWMF.h updateBCB */
static void cell_add(int *cnt, int *fw, int *bw, int i, int v)
{
    if (i) {
        if (cnt[i] == 0) {
            int nx = fw[0];
            fw[0] = i; fw[i] = nx; bw[nx] = i; bw[i] = 0;
        } else if (cnt[i] + v == 0) {
            int pv = bw[i], nx = fw[i];
            fw[pv] = nx; bw[nx] = pv;
        }
    }
    cnt[i] += v;
}

/* link feature g into the necklace of histogram row fv when its count is about to become non-zero */
static void hist_link(int *hf, int *hb, const int *row, int g)
{
    if (!row[g] && g) {
        int nx = hf[0];
        hf[g] = nx; hb[g] = 0; hf[0] = g; hb[nx] = g;
    }
}

static void hist_unlink(int *hf, int *hb, const int *row, int g)
{
    if (!row[g] && g) {
        int pv = hb[g], nx = hf[g];
        hf[pv] = nx; hb[nx] = pv;
    }
}

/* I, F: rows x cols ints (I in [0, nI), F in [0, nF)); w: nF x nF floats; out: rows x cols ints.  Returns 0. */
int jwmf_reading_core(const int *I, const int *F, const float *w, int nF, int nI, int rows, int cols, int r, int *out)
{
    int *H = calloc((size_t)nI * nF, sizeof(int)), *Hf = calloc((size_t)nI * nF, sizeof(int)), *Hb = calloc((size_t)nI * nF, sizeof(int));
    int *B = calloc(nF, sizeof(int)), *Bf = calloc(nF, sizeof(int)), *Bb = calloc(nF, sizeof(int));
    if (!H || !Hf || !Hb || !B || !Bf || !Bb) return 1;
    for (int x = 0; x < cols; ++x) {
        memset(B, 0, sizeof(int) * nF);
        memset(H, 0, sizeof(int) * (size_t)nI * nF);
        for (int i = 0; i < nI; ++i) Hf[(size_t)i * nF] = Hb[(size_t)i * nF] = 0;
        Bf[0] = Bb[0] = 0;
        int med = -1;                               /* every tap starts above the cut */
        const int x0 = x - r < 0 ? 0 : x - r, x1 = x + r > cols - 1 ? cols - 1 : x + r;
        const int y1 = r < rows - 1 ? r : rows - 1;
        for (int yy = 0; yy <= y1; ++yy)
            for (int xx = x0; xx <= x1; ++xx) {
                const int fv = I[yy * cols + xx], g = F[yy * cols + xx];
                int *row = H + (size_t)fv * nF;
                hist_link(Hf + (size_t)fv * nF, Hb + (size_t)fv * nF, row, g);
                row[g]++;
                cell_add(B, Bf, Bb, g, -1);
            }
        for (int y = 0; y < rows; ++y) {
            const float *wr = w + (size_t)F[y * cols + x] * nF;
            float bal = 0;
            int i = 0;
            do { bal += B[i] * wr[i]; i = Bf[i]; } while (i);
            if (bal >= 0) {
                for (; bal >= 0 && med; med--) {
                    float cw = 0;
                    const int *row = H + (size_t)med * nF, *rf = Hf + (size_t)med * nF;
                    int k = 0;
                    do {
                        cw += (row[k] << 1) * wr[k];
                        cell_add(B, Bf, Bb, k, -(row[k] << 1));
                        k = rf[k];
                    } while (k);
                    bal -= cw;
                }
            } else {
                for (; bal < 0 && med != nI - 1; med++) {
                    float cw = 0;
                    const int *row = H + (size_t)(med + 1) * nF, *rf = Hf + (size_t)(med + 1) * nF;
                    int k = 0;
                    do {
                        cw += (row[k] << 1) * wr[k];
                        cell_add(B, Bf, Bb, k, row[k] << 1);
                        k = rf[k];
                    } while (k);
                    bal += cw;
                }
            }
            out[y * cols + x] = bal < 0 ? med + 1 : med;
            const int ya = y + r + 1, yd = y - r;
            if (ya < rows)
                for (int xx = x0; xx <= x1; ++xx) {
                    const int fv = I[ya * cols + xx], g = F[ya * cols + xx];
                    int *row = H + (size_t)fv * nF;
                    hist_link(Hf + (size_t)fv * nF, Hb + (size_t)fv * nF, row, g);
                    row[g]++;
                    cell_add(B, Bf, Bb, g, ((fv <= med) << 1) - 1);
                }
            if (yd >= 0)
                for (int xx = x0; xx <= x1; ++xx) {
                    const int fv = I[yd * cols + xx], g = F[yd * cols + xx];
                    int *row = H + (size_t)fv * nF;
                    row[g]--;
                    hist_unlink(Hf + (size_t)fv * nF, Hb + (size_t)fv * nF, row, g);
                    cell_add(B, Bf, Bb, g, -((fv <= med) << 1) + 1);
                }
        }
    }
    free(H); free(Hf); free(Hb); free(B); free(Bf); free(Bb);
    return 0;
}

/* The whole filter for a B,G,R u8 image with at most 256 distinct 6-bit keys: identity clustering (the reference's
 * result for any RNG state), its float "exp" table with expf, then the column scan.  Returns nF, or -1 when the
 * image has more than 256 distinct keys (the clustering would be random) or on allocation failure. */
int jwmf_reading_identity(const uint8_t *img, const uint8_t *map, int rows, int cols, int r, float sigma, uint8_t *out)
{
    const int n = rows * cols;
    int *idx = calloc(1 << 18, sizeof(int)), *I = malloc(sizeof(int) * n), *F = malloc(sizeof(int) * n), *O = malloc(sizeof(int) * n);
    float *cen = malloc(sizeof(float) * 3 * 256), *w = malloc(sizeof(float) * 256 * 256);
    if (!idx || !I || !F || !O || !cen || !w) return -1;
    for (int p = 0; p < n; ++p) idx[((img[3 * p] >> 2) << 12) | ((img[3 * p + 1] >> 2) << 6) | (img[3 * p + 2] >> 2)] = 1;
    int nf = 0;
    for (int k = 0; k < (1 << 18); ++k)
        if (idx[k]) {
            if (nf == 256) { nf = -1; break; }
            cen[3 * nf] = (float)(k >> 12); cen[3 * nf + 1] = (float)((k >> 6) & 63); cen[3 * nf + 2] = (float)(k & 63);
            idx[k] = nf++;
        }
    if (nf > 0) {
        const float ns = sigma / 256.0f * 64;
        const float div = 1.0f / (2 * ns * ns);
        for (int i = 0; i < nf; ++i)
            for (int j = i; j < nf; ++j) {
                float d0 = cen[3 * i] - cen[3 * j], d1 = cen[3 * i + 1] - cen[3 * j + 1], d2 = cen[3 * i + 2] - cen[3 * j + 2];
                w[i * nf + j] = w[j * nf + i] = expf(-(d0 * d0 + d1 * d1 + d2 * d2) * div);
            }
        for (int p = 0; p < n; ++p) {
            I[p] = map[p];
            F[p] = idx[((img[3 * p] >> 2) << 12) | ((img[3 * p + 1] >> 2) << 6) | (img[3 * p + 2] >> 2)];
        }
        if (jwmf_reading_core(I, F, w, nf, 256, rows, cols, r, O)) nf = -1;
        else
            for (int p = 0; p < n; ++p) out[p] = (uint8_t)O[p];
    }
    free(idx); free(I); free(F); free(O); free(cen); free(w);
    return nf;
}
