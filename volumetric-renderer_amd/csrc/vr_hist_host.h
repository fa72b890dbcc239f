// vr_hist_host.h — the host side of include/vr/vr_hist.h: the bin edges, the bin of a value and
// the percentile window.  Plain C++ without HIP, so a stand-alone program can run it (under a
// sanitizer, tests/test_hist_cpu.py); vr_api_hist.hip includes it for vr_hist_edges, vr_hist_window
// and the edge table hist_kernel corrects its first guess against.
#pragma once

#include <stdint.h>

#include <cmath>

#include "vr_box_host.h"  // the request box: the shared rule as it is

namespace vr {

constexpr uint32_t kHistMaxBins = 4096;  // VR_HIST_MAX_BINS

// what vr_hist.h asks of (lo, hi, nbins)
inline bool hist_range_ok(float lo, float hi, uint32_t nbins)
{
    return std::isfinite(lo) && std::isfinite(hi) && lo < hi && nbins >= 1 && nbins <= kHistMaxBins;
}

// Lower edge b: left to right in double, rounded to f32 once.  b == 0 gives lo exactly.
inline float hist_edge(float lo, float hi, uint32_t nbins, uint32_t b)
{
    return (float)((double)lo + ((double)b * ((double)hi - (double)lo)) / (double)nbins);
}

inline void hist_edges(float lo, float hi, uint32_t nbins, float *e)
{
    for (uint32_t b = 0; b < nbins; ++b) e[b] = hist_edge(lo, hi, nbins, b);
}

// The first guess of v's bin, in double (the f32 form overflows where hi - lo does); the kernel
// forms the same guess from the same `scale` = nbins / (hi - lo).
inline double hist_scale(float lo, float hi, uint32_t nbins)
{
    return (double)nbins / ((double)hi - (double)lo);
}

// The bin of v, lo <= v <= hi: the largest b with e[b] <= v.  The guess is corrected against the
// edges, so the result is exact whatever the guess was.
inline uint32_t hist_bin(float v, const float *e, uint32_t nbins, float lo, double scale)
{
    double g = ((double)v - (double)lo) * scale;
    uint32_t b = g >= (double)(nbins - 1) ? nbins - 1 : (g > 0.0 ? (uint32_t)g : 0u);
    while (b + 1 < nbins && e[b + 1] <= v) ++b;
    while (b > 0 && e[b] > v) --b;
    return b;
}

// vr_hist_window's rule; false (outputs untouched) for what it refuses.
inline bool hist_window(const uint64_t *bins, uint32_t nbins, float lo, float hi, double p_lo,
                        double p_hi, float *vmin_out, float *vmax_out)
{
    if (!bins || !vmin_out || !vmax_out || !hist_range_ok(lo, hi, nbins)) return false;
    if (!(p_lo >= 0.0 && p_lo < p_hi && p_hi <= 1.0)) return false;
    uint64_t N = 0;
    for (uint32_t b = 0; b < nbins; ++b) N += bins[b];
    if (N == 0) return false;
    const uint64_t t0 = (uint64_t)std::floor(p_lo * (double)N);
    uint64_t t1 = (uint64_t)std::ceil(p_hi * (double)N);
    if (t1 < 1) t1 = 1;
    uint32_t b0 = nbins - 1, b1 = nbins - 1;
    bool have0 = false, have1 = false;
    uint64_t c = 0;
    for (uint32_t b = 0; b < nbins; ++b) {
        c += bins[b];
        if (!have0 && c > t0) {
            b0 = b;
            have0 = true;
        }
        if (!have1 && c >= t1) {
            b1 = b;
            have1 = true;
        }
    }
    *vmin_out = hist_edge(lo, hi, nbins, b0);
    *vmax_out = b1 == nbins - 1 ? hi : hist_edge(lo, hi, nbins, b1 + 1);
    return true;
}

}  // namespace vr
