// next_event_path_tracing.h — draw_next_event_path_tracing beside draw_default_path_tracing: the
// GPU engine's default path tracer (GPU/path_tracing/default_path_tracing.cu:7-34, the GPU preset:
// cap 80, the GPU hit rule) with next-event estimation, a shadow ray towards one sampled point of
// one light at every surface hit (rt_render_nee in rtmi.h).  The reference has no such renderer
// (SURVEY.md a8); its thesis shows what the direct-only flag draws
// (Descriptions/write_up/chapters/1_conceptual_background.tex:24-38, fig:direct_and_global).
// The same PathTracer (context + device scene) as draw_default_path_tracing's.
#pragma once

#include "default_path_tracing.h"

namespace rtmi {

// flags: 0 (direct + indirect light, the same expectation as the default tracer's) or
// RT_NEE_DIRECT_ONLY (the first surface's direct light alone)
inline void draw_next_event_path_tracing(SDLScreen screen, Camera& camera, std::vector<AreaLightPlane*> light_planes,
                                         std::vector<Surface*> surfaces, int spp = 32, int flags = 0) {
    static SceneArrays uploaded;
    static bool have_scene = false;
    PathTracer& pt = default_path_tracer();
    SceneArrays a = flatten(surfaces, light_planes);
    if (!have_scene || !a.same_as(uploaded)) {
        pt.set_scene(a);
        uploaded = std::move(a);
        have_scene = true;
    }
    rt_params p;
    rt_params_default(RT_PRESET_GPU, &p);
    p.width = screen.width;
    p.height = screen.height;
    p.t_scale = (float)screen.height;
    p.spp = spp;
    pt.draw_next_event(screen, camera, p, flags);  // screen shares its buffer pointer with the caller's copy
}

}  // namespace rtmi
