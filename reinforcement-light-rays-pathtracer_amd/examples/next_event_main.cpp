// next_event_main.cpp — the Cornell box by draw_next_event_path_tracing (host/next_event_path_tracing.h),
// in the shape of cornell_main.cpp: Camera(0,0,-3,1), one frame, SDL_SaveImage.
//
//   ./build/next_event_demo [out.bmp] [spp] [direct_only 0|1] [size]
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../host/camera.h"
#include "../host/next_event_path_tracing.h"
#include "../host/scene.h"
#include "../host/sdl_screen.h"

using namespace rtmi;

int main(int argc, char** argv) {
    const char* out = argc > 1 ? argv[1] : "render.bmp";
    const int spp = argc > 2 ? atoi(argv[2]) : 32;
    const int flags = (argc > 3 && atoi(argv[3]) != 0) ? RT_NEE_DIRECT_ONLY : 0;
    const int size = argc > 4 ? atoi(argv[4]) : 512;
    SDLScreen screen(size, size, false);

    std::vector<Surface> surfaces_load;
    std::vector<AreaLightPlane> light_planes_load;
    get_cornell_shapes(surfaces_load, light_planes_load);
    Camera camera(vec4(0, 0, -3, 1));

    std::vector<Surface*> surfaces;
    for (auto& s : surfaces_load) surfaces.push_back(&s);
    std::vector<AreaLightPlane*> light_planes;
    for (auto& l : light_planes_load) light_planes.push_back(&l);

    try {
        draw_next_event_path_tracing(screen, camera, light_planes, surfaces, spp, flags);
        screen.SDL_Renderframe();
    } catch (const std::exception& e) {
        fprintf(stderr, "render failed: %s\n", e.what());
        return 1;
    }
    screen.SDL_SaveImage(out);
    screen.kill_screen();
    printf("wrote %s\n", out);
    return 0;
}
