// psm_wls_tab.h - what the host forms for the WLS smoothing stage (psm_wls_filter, psm_api_wls.cpp) before a launch: the weight
// table over the 256 link indices and the lambda of every iteration.  Host only and free of HIP, so that tests/wls_tab_probe.cpp
// builds it with the host compiler; the definition is tests/wls_model.py (table, lambdas), which it equals in every bit: both go
// through the C library's exp.
#pragma once
#include <cmath>

namespace psm {

constexpr int WLS_TAB = 256;                   // link indices: the largest channel difference of two neighbouring guide pixels, 0..255
constexpr int WLS_MAX_ITERS = 4;

// tab[k] = (float)exp(-(double)k / (double)sigma)
inline void wls_table(float sigma, float tab[WLS_TAB])
{
    for (int k = 0; k < WLS_TAB; ++k) tab[k] = (float)std::exp(-(double)k / (double)sigma);
}

// lam_t = (float)((1.5 * (double)lambda * (double)4^(T-1-t)) / (double)(4^T - 1)), t = 0..T-1: Min et al.'s schedule (the
// lam_t fall by 4 from one iteration to the next and sum to lambda / 2)
inline float wls_lambda(float lambda, int T, int t)
{
    return (float)((1.5 * (double)lambda * (double)(1 << (2 * (T - 1 - t)))) / (double)((1 << (2 * T)) - 1));
}

}  // namespace psm
