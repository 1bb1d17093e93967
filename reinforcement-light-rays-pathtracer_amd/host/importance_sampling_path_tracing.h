// importance_sampling_path_tracing.h — the CPU engine's map-sampling renderer with the
// reference's name (Old_CPU_Rendering_Engine/Source/path_tracing/
// importance_sampling_path_tracing.h: draw_importance_sampling_path_tracing(screen, camera,
// radiance_map, light_planes, surfaces)), on an MI355X through the C ABI: every bounce is
// importance-sampled from the radiance map as it stands, and nothing is learned.  The CPU
// engine's map is filled by sampling the incoming radiance per sector when it is built
// (radiance_map.cpp); here RadianceMap::precompute_radiance_volumes (reinforcement_path_tracing.h,
// rt_sarsa_bake) does that on the device, for the GPU engine's 12 x 12 scalar grid.
#pragma once

#include <vector>

#include "reinforcement_path_tracing.h"

namespace rtmi {

// One frame of `spp` samples per pixel from the frozen map (RT_SARSA_TD_OFF) into the screen
// buffer; the map's TD mode is put back afterwards.  Successive calls draw fresh samples (the
// map's frame counter advances).  The scene is the one the map was built for (kept for the
// reference's argument list, which passes its light planes and surfaces).  Returns the frame's
// ray casts.
inline uint64_t draw_importance_sampling_path_tracing(SDLScreen& screen, const Camera& camera,
                                                      RadianceMap& radiance_map, const Scene& scene, int spp = 32) {
    (void)scene;
    const rt_params p = gpu_engine_params(screen, spp);
    const rt_camera cam = camera.to_rt();
    std::vector<float> rgb((size_t)screen.width * screen.height * 3);
    uint64_t casts = 0;
    int mode = RT_SARSA_TD_FRAME;
    detail::check(rt_sarsa_get_td_mode(radiance_map.handle(), &mode));
    detail::check(rt_sarsa_set_td_mode(radiance_map.handle(), RT_SARSA_TD_OFF));
    const int rc = rt_render_sarsa(radiance_map.device_scene().ctx(), radiance_map.device_scene().scene(),
                                   radiance_map.handle(), &cam, &p, 1, rgb.data(), &casts);
    const std::string e = rc != RT_OK ? rt_last_error() : "";
    detail::check(rt_sarsa_set_td_mode(radiance_map.handle(), mode));
    if (rc != RT_OK) throw std::runtime_error(e);
    screen.PutFrame(rgb.data());
    return casts;
}

}  // namespace rtmi
