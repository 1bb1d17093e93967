// rt_nee_host.cpp — next-event estimation's host-only entries (rtmi.h): the light table and the
// light sampler, by the code the kernel runs (rt_nee.hpp).  No GPU, no HIP.
#include <stdarg.h>
#include <stdio.h>

#include "../../include/rtmi.h"
#include "rt_nee.hpp"

namespace rt {
int errorf(int code, const char* fmt, ...);  // rt_capi.cpp
}

extern "C" {

int rt_nee_light_table(const float* light_v, const float* emission, int n_light, float* cdf, float* k) {
    if (n_light < 0) return rt::errorf(RT_E_INVALID, "n_light < 0 (got %d)", n_light);
    if (n_light == 0) return RT_OK;
    if (!light_v || !emission || !cdf || !k) return rt::errorf(RT_E_INVALID, "NULL argument");
    rt::nee_light_table(light_v, emission, n_light, cdf, k);
    return RT_OK;
}

int rt_nee_sample(const float* light_v, const float* cdf, int n_light, uint64_t seed, const uint32_t* pix,
                  const uint32_t* s, const int32_t* depth, int n, int32_t* light, float* y) {
    using rt::f3;
    using rt::make3;
    if (n_light < 0) return rt::errorf(RT_E_INVALID, "n_light < 0 (got %d)", n_light);
    if (n < 0) return rt::errorf(RT_E_INVALID, "n < 0 (got %d)", n);
    if (n == 0) return RT_OK;
    if ((n_light > 0 && (!light_v || !cdf)) || !pix || !s || !depth || !light || !y)
        return rt::errorf(RT_E_INVALID, "NULL argument");
    for (int l = 0; l < n_light; ++l)
        if (!(cdf[l] >= (l ? cdf[l - 1] : 0.0f)))
            return rt::errorf(RT_E_INVALID, "cdf[%d] decreases (or is not a number)", l);
    const int last = rt::nee_last_light(cdf, n_light);
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int i = 0; i < n; ++i) {
        light[i] = -1;
        y[3 * i + 0] = y[3 * i + 1] = y[3 * i + 2] = 0.0f;
        if (depth[i] < 0) return rt::errorf(RT_E_INVALID, "depth[%d] < 0 (got %d)", i, depth[i]);
        if (last < 0) continue;
        uint32_t w[4];
        rt::philox4x32_10(pix[i], s[i], 1u + (uint32_t)depth[i], rt::kNeeCounterWord, k0, k1, w);
        const int l = rt::nee_pick(cdf, last, rt::u01(w[0]));
        const float* v = light_v + (size_t)l * 9;
        // the light's hit-test record: v0, e1 = v1 - v0, e2 = v2 - v0
        const f3 p = rt::nee_point(make3(v[0], v[1], v[2]), make3(v[3] - v[0], v[4] - v[1], v[5] - v[2]),
                                   make3(v[6] - v[0], v[7] - v[1], v[8] - v[2]), rt::u01(w[1]), rt::u01(w[2]));
        light[i] = l;
        y[3 * i + 0] = p.x;
        y[3 * i + 1] = p.y;
        y[3 * i + 2] = p.z;
    }
    return RT_OK;
}

}  // extern "C"
