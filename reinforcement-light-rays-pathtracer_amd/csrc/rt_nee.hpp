// rt_nee.hpp — next-event estimation's light sampler (rtmi.h "next-event estimation"): what the
// kernel k_render_nee (rt_nee.hip) and the host entries rt_nee_light_table / rt_nee_sample
// (rt_nee_host.cpp) share.  Every function evaluates the same binary32 operations in the same
// order on host and device (rt_math.hpp's rules: -ffp-contract=off, IEEE / and sqrt).
#pragma once

#include <math.h>

#include "rt_math.hpp"

namespace rt {

constexpr uint32_t kNeeCounterWord = 0x4E454531u;  // "NEE1": word 3 of the direct term's Philox counter

// A light's weight area (Le.r + Le.g + Le.b) in double, and *le = Le.r + Le.g + Le.b.  A weight that
// is not a positive number (no area, no or negative emission, a NaN) counts as 0.
inline double nee_light_weight(const float* v, const float* e, double* le) {
    const double e1[3] = {(double)v[3] - v[0], (double)v[4] - v[1], (double)v[5] - v[2]};
    const double e2[3] = {(double)v[6] - v[0], (double)v[7] - v[1], (double)v[8] - v[2]};
    const double cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2],
                 cz = e1[0] * e2[1] - e1[1] * e2[0];
    *le = ((double)e[0] + (double)e[1]) + (double)e[2];
    const double w = (0.5 * sqrt((cx * cx + cy * cy) + cz * cz)) * *le;
    return w > 0.0 ? w : 0.0;
}

// The light table of n lights (triangles [n][9], emission [n][3]), built in double and stored as
// float: w_l = area_l (Le.r + Le.g + Le.b), cdf[l] = (w_0 + .. + w_l) / sum in index order,
// k[l] = sum / (Le.r + Le.g + Le.b), the reciprocal of the area pdf; k = 0 for a light of weight 0.
// A list without weight: zeros.
inline void nee_light_table(const float* light_v, const float* emission, int n, float* cdf, float* k) {
    double sum = 0.0, le = 0.0;
    for (int l = 0; l < n; ++l) sum += nee_light_weight(light_v + (size_t)l * 9, emission + (size_t)l * 3, &le);
    double run = 0.0;
    for (int l = 0; l < n; ++l) {
        const double w = nee_light_weight(light_v + (size_t)l * 9, emission + (size_t)l * 3, &le);
        run += w;
        cdf[l] = sum > 0.0 ? (float)(run / sum) : 0.0f;
        k[l] = w > 0.0 ? (float)(sum / le) : 0.0f;
    }
}

// The light that catches what no boundary does: the last one whose cdf exceeds its
// predecessor's (a table of nee_light_table: the last light with weight), -1: no light has weight.
inline int nee_last_light(const float* cdf, int n) {
    int last = -1;
    float prev = 0.0f;
    for (int l = 0; l < n; ++l) {
        if (cdf[l] > prev) last = l;
        prev = cdf[l];
    }
    return last;
}

// The first light l <= last with r < cdf[l], else last (cdf does not decrease; last >= 0).
RT_HD int nee_pick(const float* cdf, int last, float r) {
    int lo = 0, hi = last;  // the answer lies in [lo, hi]
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (r < cdf[mid])
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// The point of the light triangle (v0, e1 = v1 - v0, e2 = v2 - v0) for the uniforms (u, v):
// folded into the triangle, y = (v0 + u e1) + v e2.
RT_HD f3 nee_point(f3 v0, f3 e1, f3 e2, float u, float v) {
    if (u + v > 1.0f) {
        u = 1.0f - u;
        v = 1.0f - v;
    }
    return make3((v0.x + u * e1.x) + v * e2.x, (v0.y + u * e1.y) + v * e2.y, (v0.z + u * e1.z) + v * e2.z);
}

// The geometry of the direct term at pos on a surface of normal N towards the point y of a light of
// normal Nl: false = no cast and no contribution (cx <= 0, cy == 0 or d2 == 0).  *d: the unit
// direction, *g = (cx cy) / d2, to be multiplied by the light's k.
RT_HD bool nee_geometry(f3 pos, f3 N, f3 y, f3 Nl, f3* d, float* g) {
    const f3 Lv = make3(y.x - pos.x, y.y - pos.y, y.z - pos.z);
    const float d2 = dot(Lv, Lv);
    if (d2 == 0.0f) return false;
    *d = normalize(Lv);
    const float cx = dot(N, *d);
    const float cy = fabsf(dot(Nl, *d));
    if (!(cx > 0.0f) || !(cy > 0.0f)) return false;  // cx <= 0 or cy == 0 (or not a number)
    *g = (cx * cy) / d2;
    return true;
}

}  // namespace rt
