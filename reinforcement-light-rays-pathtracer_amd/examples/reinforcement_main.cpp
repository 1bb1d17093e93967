// reinforcement_main.cpp — the GPU engine's learned-sampling main loops
// (GPU/main.cu:260-350 Expected SARSA, :420-470 pre-trained DQN) written against
// the drop-in facade: load a scene, render frames, log the per-frame statistics and
// append them to sarsa_training_stats.txt (the format of Radiance_Map_Data/sarsa_*.txt),
// save the Q-table (radiance_map_data.txt) and the last frame, in the working directory.
//
//   ./build/reinforcement_demo sarsa <scene.obj> <kind> [frames] [spp] [out.bmp]
//   ./build/reinforcement_demo dqn <scene.obj> <kind> <model> [frames] [spp] [out.bmp]
//   ./build/reinforcement_demo neuralq <scene.obj> <kind> <model> [frames] [spp] [out.bmp]
//     (trains from <model>; writes nn_training_stats.txt and trained.model)
//   ./build/reinforcement_demo voronoi <scene.obj> <kind> [frames] [out.bmp] [width height]
//     (GPU/main.cu:414-495, PATH_TRACING_METHOD 2: the radiance volumes' Voronoi view, one
//      sample per frame; the last frame is saved)
//   ./build/reinforcement_demo importance <scene.obj> <kind> [frames] [spp] [out.bmp] [width height] [bake_spp]
//     (the CPU engine's importance-sampling renderer, Old_CPU_Rendering_Engine/Source/main.cpp:
//      the radiance map filled from ground truth, bake_spp paths per sector (0: left as
//      created), then frames rendered from the frozen map; the last frame is saved)
//   ./build/reinforcement_demo irradiance <scene.obj> <kind> [frames] [bake_spp] [out.bmp] [width height] [k]
//     (the CPU engine's irradiance render of the map, draw_radiance_map_path_tracing: the map
//      filled from ground truth, bake_spp paths per sector, then each camera hit drawn as the
//      average estimate of its k closest volumes; one sample per frame, the last frame is saved)
//   ./build/reinforcement_demo sweep <scene.obj> <kind> [frames] [spp] [out.bmp] [width height] [sweeps] [sweep_spp]
//     (value iteration over the radiance map, rt_sarsa_sweep: `sweeps` sweeps of sweep_spp casts
//      per sector, each with fresh samples and averaged with the ones before, then frames rendered
//      from the frozen map; the last frame is saved)
//   (kind: 1 door_room, 2 archway, 3 complex_light_room; scene "cornell" = the Cornell box)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "../host/camera.h"
#include "../host/importance_sampling_path_tracing.h"
#include "../host/precompute_irradiance_path_tracing.h"
#include "../host/reinforcement_path_tracing.h"
#include "../host/scene.h"
#include "../host/sdl_screen.h"
#include "../host/voronoi_trace.h"

using namespace rtmi;

static vec4 camera_for(int kind) {  // GPU/main.cu:100-104
    switch (kind) {
        case 1: return vec4(0.f, 0.5f, -0.9f, 1.f);
        case 2: return vec4(-1.f, 0.2f, -0.99f, 1.f);
        case 3: return vec4(-1.f, -1.f, -0.4f, 1.f);
        default: return vec4(0.f, 0.f, -3.f, 1.f);
    }
}

int main(int argc, char** argv) {
    if (argc < 4) {
        fprintf(stderr, "usage: %s sarsa|dqn|neuralq|voronoi|importance|irradiance|sweep <scene.obj|cornell> <kind> [model] [frames] [spp] [out.bmp]\n", argv[0]);
        return 2;
    }
    const bool nq = strcmp(argv[1], "neuralq") == 0;
    const bool dqn = nq || strcmp(argv[1], "dqn") == 0;
    const int kind = atoi(argv[3]);
    int a = 4;
    const char* model = dqn ? (argc > a ? argv[a++] : "") : "";
    const bool voronoi = strcmp(argv[1], "voronoi") == 0;
    const int frames = argc > a ? atoi(argv[a++]) : 4;
    const int spp = (!voronoi && argc > a) ? atoi(argv[a++]) : 32;
    const char* out = argc > a ? argv[a++] : "render.bmp";
    const bool importance = strcmp(argv[1], "importance") == 0;
    const bool irradiance = strcmp(argv[1], "irradiance") == 0;  // (its spp argument is bake_spp)
    const bool sweep = strcmp(argv[1], "sweep") == 0;
    const bool sized = (voronoi || importance || irradiance || sweep) && argc > a + 1;
    const int width = sized ? atoi(argv[a]) : 512;
    const int height = sized ? atoi(argv[a + 1]) : 512;
    const int bake_spp = (importance && argc > a + 2) ? atoi(argv[a + 2]) : 64;
    const int sweeps = (sweep && argc > a + 2) ? atoi(argv[a + 2]) : 7;
    const int sweep_spp = (sweep && argc > a + 3) ? atoi(argv[a + 3]) : 8;
    const int query_count = (irradiance && argc > a + 2) ? atoi(argv[a + 2]) : 3;
    if (width <= 0 || height <= 0) {
        fprintf(stderr, "bad screen size %d x %d\n", width, height);
        return 2;
    }
    Scene scene;
    if (strcmp(argv[2], "cornell") == 0) scene.load_cornell_box_scene();
    else if (!scene.load_custom_scene_kind(argv[2], kind)) {
        fprintf(stderr, "cannot load %s\n", argv[2]);
        return 1;
    }
    SDLScreen screen(width, height, false);
    Camera camera(camera_for(kind));
    try {
        DeviceScene ds(scene);
        if (nq) {
            NeuralQPathtracer pt(ds, model);
            for (int f = 0; f < frames; ++f) {
                const uint64_t casts = pt.render_frame(screen, camera, spp);
                printf("frame %d: %llu ray casts, epsilon %.3f\n", f, (unsigned long long)casts, pt.epsilon());
            }
            pt.save_model("trained.model");
        } else if (voronoi) {
            // GPU/main.cu:429-490: the radiance map, its Voronoi colours, then the render loop
            RadianceMap map(ds);
            printf("radiance volumes: %d (KD array %d)\n", map.radiance_volumes_count, map.radiance_array_size);
            map.set_voronoi_colours();
            for (int f = 0; f < frames; ++f) {
                draw_voronoi_trace(screen, map, camera, scene, (uint32_t)f);
                printf("frame %d: voronoi view\n", f);
            }
        } else if (importance) {
            RadianceMap map(ds);
            printf("radiance volumes: %d (KD array %d)\n", map.radiance_volumes_count, map.radiance_array_size);
            if (bake_spp > 0) {
                const uint64_t casts = map.precompute_radiance_volumes(bake_spp, bake_spp % 4 == 0 ? 4 : 1, height);
                printf("precomputed %d paths per sector: %llu ray casts\n", bake_spp, (unsigned long long)casts);
            }
            for (int f = 0; f < frames; ++f) {
                const uint64_t casts = draw_importance_sampling_path_tracing(screen, camera, map, scene, spp);
                printf("frame %d: importance sampling, average path length %.3f\n", f,
                       (double)casts / ((double)screen.width * screen.height * spp));
            }
        } else if (sweep) {
            RadianceMap map(ds);
            printf("radiance volumes: %d (KD array %d)\n", map.radiance_volumes_count, map.radiance_array_size);
            for (int k = 0; k < sweeps; ++k) {
                const uint64_t casts = map.sweep(sweep_spp, (uint32_t)(k * sweep_spp), true, height);
                printf("sweep %d: %d casts per sector, %llu ray casts\n", k, sweep_spp, (unsigned long long)casts);
            }
            for (int f = 0; f < frames; ++f) {
                const uint64_t casts = draw_importance_sampling_path_tracing(screen, camera, map, scene, spp);
                printf("frame %d: swept map, average path length %.3f\n", f,
                       (double)casts / ((double)screen.width * screen.height * spp));
            }
        } else if (irradiance) {
            RadianceMap map(ds);
            printf("radiance volumes: %d (KD array %d)\n", map.radiance_volumes_count, map.radiance_array_size);
            const uint64_t casts = map.precompute_radiance_volumes(spp, spp % 4 == 0 ? 4 : 1, height);
            printf("precomputed %d paths per sector: %llu ray casts\n", spp, (unsigned long long)casts);
            for (int f = 0; f < frames; ++f) {
                draw_radiance_map_path_tracing(screen, map, camera, scene, query_count, (uint32_t)f);
                printf("frame %d: irradiance view, %d closest volumes\n", f, query_count);
            }
        } else if (dqn) {
            PretrainedPathtracer pt(ds, model);
            for (int f = 0; f < frames; ++f) {
                const uint64_t casts = pt.render_frame(screen, camera, spp);
                printf("frame %d: average path length %.3f\n", f,
                       (double)casts / ((double)screen.width * screen.height * spp));
            }
        } else {
            RadianceMap map(ds);
            printf("radiance volumes: %d (KD array %d)\n", map.radiance_volumes_count, map.radiance_array_size);
            for (int f = 0; f < frames; ++f) {
                const uint64_t casts = draw_reinforcement_path_tracing(screen, camera, map, spp);
                printf("frame %d: average path length %.3f\n", f,
                       (double)casts / ((double)screen.width * screen.height * spp));
                // GPU/main.cu:321-339: the logged statistics and the training-stats line
                float avg = 0.f;
                uint64_t zero = 0;
                map.frame_stats(screen.width * screen.height, &avg, &zero);
                printf("Average Path Length: %.3f\n", avg);
                printf("Zero contribution light paths: %llu\n", (unsigned long long)zero);
                map.append_training_stats("sarsa_training_stats.txt", screen.width * screen.height);
                update_radiance_volume_distributions(map);
            }
            map.save_q_vals_to_file("radiance_map_data.txt");  // SAVE_RADIANCE_MAP (main.cu:353-369)
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "render failed: %s\n", e.what());
        return 1;
    }
    screen.SDL_Renderframe();
    screen.SDL_SaveImage(out);
    screen.kill_screen();
    printf("wrote %s\n", out);
    return 0;
}
