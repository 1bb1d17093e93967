// voronoi_trace.h — the GPU engine's Voronoi view with the reference's name
// (GPU/path_tracing/voronoi_trace.cuh; host loop GPU/main.cu:414-495, PATH_TRACING_METHOD 2):
// every camera hit in the colour of its nearest radiance volume, lights and misses white.
// RadianceMap::set_voronoi_colours() (reinforcement_path_tracing.h) draws the random colours.
#pragma once

#include <vector>

#include "reinforcement_path_tracing.h"

namespace rtmi {

// draw_voronoi_trace (voronoi_trace.cu:4-38) for one frame of one sample per pixel into the
// screen buffer.  frame: the sample index of the frame's camera rays (the reference's
// curand state moves on from frame to frame, so each frame re-jitters).  The scene is the
// one the map was built for (kept for the reference's argument list).
inline void draw_voronoi_trace(SDLScreen& screen, RadianceMap& radiance_map, const Camera& camera, const Scene& scene,
                               uint32_t frame = 0) {
    (void)scene;
    const rt_params p = gpu_engine_params(screen, 1);
    const rt_camera cam = camera.to_rt();
    std::vector<float> rgb((size_t)screen.width * screen.height * 3);
    detail::check(rt_render_volume_view(radiance_map.device_scene().ctx(), radiance_map.device_scene().scene(),
                                        radiance_map.handle(), &cam, &p, frame, rgb.data(), nullptr, nullptr,
                                        nullptr));
    screen.PutFrame(rgb.data());
}

}  // namespace rtmi
