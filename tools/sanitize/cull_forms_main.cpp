// cull_forms_main.cpp — the two halves of the primary-ray cull (csrc/rt_cull.hpp) against its
// definition, on the host under the sanitizers, with no GPU: a stand-alone program.  The forms
// go through a heap buffer of exactly the device buffer's size, written as k_cull_forms writes
// it (one "thread" per column, zeros past the scene) and read as a cull wave reads it (lane i of
// word g reads column 64 g + i, whatever n_tri is), so an index outside it is an
// AddressSanitizer report.
//
//   c++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -D__HIP_PLATFORM_AMD__ -I$ROCM/include tools/sanitize/cull_forms_main.cpp -o cull_forms_san && ./cull_forms_san
//
// Prints "cull_forms: ok" and exits 0 when every comparison holds and no sanitizer fired.
#include <hip/hip_runtime_api.h>

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <random>
#include <vector>

#include "../../reinforcement-light-rays-pathtracer_amd/csrc/rt_cull.hpp"

namespace {
int g_bad = 0;
void expect(bool ok, const char* what, int a, int b) {
    if (!ok && g_bad++ < 10) fprintf(stderr, "cull_forms: %s differs (case %d, %d)\n", what, a, b);
}
bool same_bits(const rt::CamRect& a, const rt::CamRect& b) { return memcmp(&a, &b, sizeof(a)) == 0; }
}  // namespace

int main() {
    std::mt19937 rng(20240611u);
    std::uniform_real_distribution<float> coord(-2.0f, 2.0f), small(0.0f, 1e-4f), yaw(-1.5f, 1.5f);
    const int frames[][2] = {{512, 512}, {40, 24}, {17, 33}, {1, 1}, {2048, 64}};
    int n_culled[2] = {0, 0}, n_kept[2] = {0, 0};
    for (int round = 0; round < 40; ++round) {
        const int n_tri = (round == 0) ? 1 : (round == 1) ? rt::kCullFormStride : 1 + (int)(rng() % rt::kCullFormStride);
        // filter records: direction-like rows in [-2, 2], margins small and positive (w of rows 1..3)
        std::vector<float4> filt((size_t)n_tri * rt::kFiltF4);
        for (int i = 0; i < n_tri; ++i)
            for (int k = 0; k < rt::kFiltF4; ++k)
                filt[(size_t)i * rt::kFiltF4 + k] =
                    make_float4(coord(rng), coord(rng), coord(rng), (k >= 1 && k <= 3) ? small(rng) : coord(rng));
        const int W = frames[round % 5][0], H = frames[round % 5][1];
        const float y = (round % 7 == 0) ? 0.0f : yaw(rng);
        const float cx = coord(rng), cy = coord(rng), cz = coord(rng) - 3.0f;
        const float cosy = cosf(y), siny = sinf(y), ts = (round & 1) ? 512.0f : 1.0f;
        const rt::CamConst k = rt::make_cam_const(cx, cy, cz, cosy, siny, W, H, ts);
        // the device buffer, as k_cull_forms fills it
        float4* forms = new float4[(size_t)rt::kCullFormRows * rt::kCullFormStride];
        for (int t = 0; t < rt::kCullFormStride; ++t) {
            float4 r[rt::kCullFormRows];
            if (t < n_tri) {
                rt::cull_forms_rows(rt::cull_forms(&filt[(size_t)t * rt::kFiltF4], k), r);
            } else {
                for (int j = 0; j < rt::kCullFormRows; ++j) r[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
            for (int j = 0; j < rt::kCullFormRows; ++j) forms[j * rt::kCullFormStride + t] = r[j];
        }
        for (int rc = 0; rc < 60; ++rc) {
            int x0 = (int)(rng() % W), x1 = (int)(rng() % W), y0 = (int)(rng() % H), y1 = (int)(rng() % H);
            if (x0 > x1) std::swap(x0, x1);
            if (y0 > y1) std::swap(y0, y1);
            if (rc == 0) { x0 = y0 = 0; x1 = W - 1; y1 = H - 1; }
            if (rc % 3 == 1) { x1 = x0; y1 = y0; }  // single pixels, the bench's shape
            const rt::CamRect want_c = rt::make_cam_rect(cx, cy, cz, cosy, siny, W, H, ts, x0, x1, y0, y1);
            const rt::CamRect c = rt::cam_rect_of(k, x0, x1, y0, y1);
            expect(same_bits(c, want_c), "CamRect", round, rc);
            for (int g = 0; g < rt::kRenderCullWords && g * 64 < n_tri; ++g) {
                for (int lane = 0; lane < 64; ++lane) {
                    const int i = g * 64 + lane;
                    float4 r[rt::kCullFormRows];
                    for (int j = 0; j < rt::kCullFormRows; ++j) r[j] = forms[j * rt::kCullFormStride + i];
                    const rt::CullForms o = rt::cull_forms_of_rows(r);
                    const bool got0 = rt::rect_cull_forms<0>(o, c), got1 = rt::rect_cull_forms<1>(o, c);
                    if (i >= n_tri) continue;  // (the kernel masks these lanes off)
                    const bool w0 = rt::rect_cull<0>(&filt[(size_t)i * rt::kFiltF4], want_c);
                    const bool w1 = rt::rect_cull<1>(&filt[(size_t)i * rt::kFiltF4], want_c);
                    expect(got0 == w0, "rect_cull<0>", round, i);
                    expect(got1 == w1, "rect_cull<1>", round, i);
                    (w0 ? n_culled : n_kept)[0]++;
                    (w1 ? n_culled : n_kept)[1]++;
                }
            }
        }
        delete[] forms;
    }
    printf("cull_forms: rule 0 culled %d kept %d, rule 1 culled %d kept %d\n", n_culled[0], n_kept[0], n_culled[1],
           n_kept[1]);
    if (g_bad || !n_culled[0] || !n_kept[0] || !n_culled[1] || !n_kept[1]) {
        fprintf(stderr, "cull_forms: FAILED (%d mismatches, or one answer never seen)\n", g_bad);
        return 1;
    }
    printf("cull_forms: ok\n");
    return 0;
}
