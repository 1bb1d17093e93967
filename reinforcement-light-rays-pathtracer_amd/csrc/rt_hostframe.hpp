// rt_hostframe.hpp — what the whole-rectangle entries with host buffers share (host only):
// rt_render, rt_cull_masks_device, rt_render_sarsa, rt_render_volume_view, rt_render_irradiance,
// rt_render_glyph_view, rt_render_dqn, rt_render_dqn_view.  HostFrame owns the device side of one
// such call -- the 16 x 16 block list of the rectangle and a device buffer per output that was
// asked for --; the parameter checks the entries have in common stand below it.
#pragma once

#include <string>
#include <vector>

#include "rt_internal.hpp"

namespace rt {

class HostFrame {
public:
    // the blocks of the rectangle (x0, y0, w, h) of the image, row by row; a block's output
    // origin is its offset in the rectangle
    HostFrame(int x0, int y0, int w, int h) {
        for (int by = 0; by < h; by += 16)
            for (int bx = 0; bx < w; bx += 16) blocks_.push_back({x0 + bx, y0 + by, bx, by});
    }
    ~HostFrame() {
        (void)hipFree(d_blocks_);
        for (Buf& b : bufs_) (void)hipFree(b.dev);
    }
    HostFrame(const HostFrame&) = delete;
    HostFrame& operator=(const HostFrame&) = delete;

    // An output of `bytes`: where host is not NULL, begin() allocates a device buffer into *dev
    // (fill >= 0: set to that byte first) and finish() copies it back to host.
    template <class T>
    void out(T** dev, void* host, size_t bytes, int fill = -1) {
        *dev = nullptr;
        if (host) bufs_.push_back({dev, &set_slot<T>, nullptr, host, nullptr, bytes, fill});
    }
    // an input of `bytes`, uploaded by begin() where host is not NULL
    template <class T>
    void in(T** dev, const void* host, size_t bytes) {
        *dev = nullptr;
        if (host) bufs_.push_back({dev, &set_slot<T>, nullptr, nullptr, host, bytes, -1});
    }
    int n_blocks() const { return (int)blocks_.size(); }
    const BlockDesc* blocks() const { return d_blocks_; }  // (after begin)

    // allocates what was asked for, uploads the blocks and the inputs, fills
    hipError_t begin() {
        hipError_t e = hipMalloc(&d_blocks_, sizeof(BlockDesc) * blocks_.size());
        for (Buf& b : bufs_) {
            if (e == hipSuccess) e = hipMalloc(&b.dev, b.bytes);
            if (e == hipSuccess) b.set(b.slot, b.dev);
        }
        if (e == hipSuccess)
            e = hipMemcpy(d_blocks_, blocks_.data(), sizeof(BlockDesc) * blocks_.size(), hipMemcpyHostToDevice);
        for (Buf& b : bufs_) {
            if (e == hipSuccess && b.src) e = hipMemcpy(b.dev, b.src, b.bytes, hipMemcpyHostToDevice);
            if (e == hipSuccess && b.fill >= 0) e = hipMemset(b.dev, b.fill, b.bytes);
        }
        return e;
    }
    // After the caller's launches (rc: their code, e: begin's or their HIP error): synchronises
    // and copies the outputs back.  rc first, then RT_E_HIP "<entry>: <hip error string>".
    int finish(int rc, hipError_t e, const char* entry) {
        if (rc != RT_OK) return rc;
        if (e == hipSuccess) e = hipDeviceSynchronize();
        for (Buf& b : bufs_)
            if (e == hipSuccess && b.dst) e = hipMemcpy(b.dst, b.dev, b.bytes, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return set_error(RT_E_HIP, (std::string(entry) + ": " + hipGetErrorString(e)).c_str());
        return RT_OK;
    }

private:
    // the caller's device pointer is written as what it is (a T*), not through a void**
    template <class T>
    static void set_slot(void* slot, void* dev) {
        *static_cast<T**>(slot) = static_cast<T*>(dev);
    }
    struct Buf {
        void* slot;  // the caller's device pointer (a T**), set by `set`
        void (*set)(void* slot, void* dev);
        void* dev;
        void* dst;        // host: copied back (an output)
        const void* src;  // host: uploaded (an input)
        size_t bytes;
        int fill;
    };
    std::vector<BlockDesc> blocks_;
    BlockDesc* d_blocks_ = nullptr;
    std::vector<Buf> bufs_;
};

// ---- the parameter checks the entries share (each entry keeps its own order and its other refusals) ----
inline bool params_size_bad(const rt_params* p) { return p->width <= 0 || p->height <= 0 || p->spp <= 0; }
// spp_split and the image size, in this order: NULL, or the text of the RT_E_INVALID refusal
inline const char* params_split_refusal(const rt_params* p) {
    const int split = p->spp_split <= 0 ? 1 : p->spp_split;
    if (split > 64 || (split & (split - 1)) != 0) return "spp_split must be a power of two <= 64";
    if (p->spp % split != 0) return "spp_split does not divide spp";
    if ((int64_t)p->width * (int64_t)p->height > (int64_t)1 << 31) return "image too large";
    return nullptr;
}

}  // namespace rt
