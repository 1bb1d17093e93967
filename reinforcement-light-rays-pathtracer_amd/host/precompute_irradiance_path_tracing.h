// precompute_irradiance_path_tracing.h -- the CPU engine's irradiance render of a radiance map
// with the reference's name (Old_CPU_Rendering_Engine/Source/path_tracing/
// precompute_irradiance_path_tracing.cpp:3-53): one camera ray per pixel, no bounce; a surface
// hit is drawn as the map's own irradiance estimate there, the average over the closest
// radiance volumes (RadianceMap::get_irradiance_estimate, radiance_map.cpp:93-128) times the
// surface's colour; a light as its emission, a miss black.
// RadianceMap::precompute_radiance_volumes() (reinforcement_path_tracing.h) fills the map first.
#pragma once

#include <vector>

#include "reinforcement_path_tracing.h"

namespace rtmi {

// draw_radiance_map_path_tracing for one frame of one sample per pixel into the screen buffer.
// closest_query_count: CLOSEST_QUERY_COUNT (constants/radiance_volumes_settings.h:14), the
// volumes averaged per hit, at most RT_SARSA_KNN_MAX; the search radius is the map's reach
// (RadianceMap::max_query_dist; the reference's MAX_DIST 0.5 is beyond what the grid answers).
// frame: the sample index of the frame's camera rays (each frame re-jitters).  The scene is the
// one the map was built for (kept for the reference's argument list).
inline void draw_radiance_map_path_tracing(SDLScreen& screen, RadianceMap& radiance_map, const Camera& camera,
                                           const Scene& scene, int closest_query_count = 1, uint32_t frame = 0) {
    (void)scene;
    const rt_params p = gpu_engine_params(screen, 1);
    const rt_camera cam = camera.to_rt();
    const rt_irr_opts o = {closest_query_count, radiance_map.max_query_dist(), RT_IRR_MEAN, 1};
    std::vector<float> rgb((size_t)screen.width * screen.height * 3);
    detail::check(rt_render_irradiance(radiance_map.device_scene().ctx(), radiance_map.device_scene().scene(),
                                       radiance_map.handle(), &cam, &p, &o, frame, rgb.data(), nullptr, nullptr, nullptr,
                                       nullptr));
    screen.PutFrame(rgb.data());
}

}  // namespace rtmi
