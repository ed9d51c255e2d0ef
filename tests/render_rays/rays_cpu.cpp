// rays_cpu.cpp — the per-ray functions of trt_render_rays (csrc/trt_path.h: rayRecord, rayValid, cameraRecord) compiled for the host, for
// tests/test_render_rays_cpu.py: the same code k_rays_pack and the camera-ray generators wrap.
#include <cstring>

#include "trt_path.h"

using namespace trtd;

extern "C" {

// The queue record cameraRecord() writes for (pixel y * width + x, sample) of `cam` as path `pid` -> cam_rec[8], and the record rayRecord()
// writes for that record's own ray -> ray_rec[8] (ra.xyzw, rb.xyzw as raw 32-bit words).
void rays_cpu_records(const trt_camera* cam, int width, int height, uint32_t seed, int fixed, int y, int x, uint32_t sample, uint32_t pid, uint32_t* cam_rec,
                      uint32_t* ray_rec)
{
    SceneDev sc;
    std::memset(&sc, 0, sizeof(sc));
    sc.cam = *cam;
    TileDesc td;
    std::memset(&td, 0, sizeof(td));
    td.width = width;
    td.height = height;
    td.seed = seed;
    td.fixed_pixels = fixed ? 1u : 0u;
    f4 ra, rb;
    cameraRecord(sc, td, y, x, sample, pid, ra, rb);
    std::memcpy(cam_rec, &ra, 16);
    std::memcpy(cam_rec + 4, &rb, 16);
    f4 qa, qb;
    rayRecord(mk3(ra.x, ra.y, ra.z), mk3(ra.w, rb.x, rb.y), pid, qa, qb);
    std::memcpy(ray_rec, &qa, 16);
    std::memcpy(ray_rec + 4, &qb, 16);
}

// the fields of a record's state word: {next draw, ray type, depth}
void rays_cpu_meta(uint32_t meta, uint32_t* out)
{
    out[0] = metaCtr(meta);
    out[1] = metaType(meta);
    out[2] = metaDepth(meta);
}

// rayValid() on n rays given as raw words org[n][3], dir[n][3] -> valid[n]
void rays_cpu_valid(const uint32_t* org, const uint32_t* dir, uint32_t n, uint8_t* valid)
{
    for (uint32_t i = 0; i < n; ++i) {
        float o[3], d[3];
        std::memcpy(o, org + 3 * (size_t)i, 12);
        std::memcpy(d, dir + 3 * (size_t)i, 12);
        valid[i] = rayValid(ld3(o), ld3(d)) ? 1 : 0;
    }
}

}  // extern "C"
