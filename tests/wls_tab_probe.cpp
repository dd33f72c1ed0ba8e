// wls_tab_probe.cpp - the host-only header of the WLS smoothing stage (primestereomatch_amd/csrc/psm_wls_tab.h) behind ctypes:
// tests/test_wls_tab.py builds it with the host compiler and compares the weight table and the per-iteration lambdas with
// tests/wls_model.py, bit for bit.  With -DWLS_TAB_PROBE_MAIN it is a program of its own (for a sanitizer build).
#include "../primestereomatch_amd/csrc/psm_wls_tab.h"

#include <cstdio>

extern "C" {

int wls_probe_entries() { return psm::WLS_TAB; }
int wls_probe_max_iters() { return psm::WLS_MAX_ITERS; }
void wls_probe_table(float sigma, float *tab) { psm::wls_table(sigma, tab); }
float wls_probe_lambda(float lambda, int T, int t) { return psm::wls_lambda(lambda, T, t); }

}  // extern "C"

#ifdef WLS_TAB_PROBE_MAIN
int main()
{
    const float sigmas[] = {0.5f, 1.5f, 37.25f, 1e-3f, 1e6f};
    float tab[psm::WLS_TAB];
    double sum = 0.0;
    for (float s : sigmas) {
        psm::wls_table(s, tab);
        for (int k = 0; k < psm::WLS_TAB; ++k) sum += tab[k];
    }
    for (int T = 1; T <= psm::WLS_MAX_ITERS; ++T)
        for (int t = 0; t < T; ++t) sum += psm::wls_lambda(8000.0f, T, t);
    printf("5 tables, 10 lambdas, sum %.6f\n", sum);
    return 0;
}
#endif
