// trt_despeckle.h — the per-pixel arithmetic of trt_despeckle (include/trt.h): the firefly clamp that runs on a frame before the history
// and the filter see it.  Written once for the kernel (trt_despeckle_kernels.h) and for its CPU build (tests/despeckle).  Demodulation and
// luminance are trt_denoise.h's functions, so the clamp works in the domain the filter and the history work in.  Plain fp32 operations in
// one fixed order, no contraction on either side (-ffp-contract=off), the root by trt_sqrt: hipcc for gfx950 and g++ on x86-64 give the
// same bits.
//
// Pixels are read through a fetch object: f(x, y) = the demodulated luminance of pixel (x, y) if that pixel is in the image and a hit, NaN
// otherwise.  A luminance that is not finite does not count either, so "the tap counts" is trt_ds_finite(f(x, y)) for every fetch: global
// memory (trt_ds_frame), or a tile of luminances in LDS.
#ifndef TRT_DESPECKLE_H
#define TRT_DESPECKLE_H

#include "trt_denoise.h"

#define TRT_DS_RADIUS 1
#define TRT_DS_SIGMA 3.0f

// trt_despeckle_params with its defaults filled in.
struct trt_ds_args {
    int width, height;
    int radius;   // 1 or 2
    float sigma;  // k
};

// Every check of include/trt.h that needs no device, in its order, for the entry points and the CPU build alike.  required = color, albedo,
// depth and out_color are there; paired = variance and out_variance are both there or both not.  Fills `a`.  nullptr, or what is wrong.
static inline const char* trt_ds_check(const trt_despeckle_params* p, int width, int height, bool required, bool paired, trt_ds_args& a)
{
    if (!required) return "null buffer";
    if (!paired) return "variance and out_variance: both or neither";
    if (width < 1 || height < 1) return "width and height must be >= 1";
    if ((unsigned long long)width * (unsigned long long)height > TRT_DENOISE_MAX_PIXELS) return "image larger than 2^28 pixels";
    trt_despeckle_params d{};
    if (p) d = *p;
    if (d.radius < 0 || d.radius > 2) return "radius must be 0, 1 or 2";
    if (!(d.sigma >= 0.0f)) return "sigma must be >= 0";
    if (d.flags != 0) return "flags must be 0";
    a.width = width;
    a.height = height;
    a.radius = d.radius ? d.radius : TRT_DS_RADIUS;
    a.sigma = d.sigma != 0.0f ? d.sigma : TRT_DS_SIGMA;
    return nullptr;
}

// Neither a NaN nor an infinity.
static inline TRT_HD bool trt_ds_finite(float v) { return fabsf(v) <= 3.4028234663852886e38f; }

static inline TRT_HD float trt_ds_nan() { return __builtin_nanf(""); }

// Step 1 for one pixel: l = lum(color / a); NaN for a miss (a tap that is a miss does not count, and NaN is how the fetches say so).
static inline TRT_HD float trt_ds_luminance(const float* color, const float* albedo, float depth)
{
    if (!trt_dn_hit(depth)) return trt_ds_nan();
    const trt_dn4 a = trt_dn_factor(albedo[0], albedo[1], albedo[2]);
    const trt_dn4 c = trt_dn_demodulate(color[0], color[1], color[2], 0.0f, a);
    return trt_dn_lum(c.x, c.y, c.z);
}

struct trt_ds_pixel_out {
    float color[3];
    float variance;
    float scale;
};

// Steps 1 to 9 at the pixel (x, y) with the given colour, albedo, depth and variance (0 when the call has none).  Taps in the order
// dy = -R..R (rows), dx = -R..R, the centre left out.
template <int R, class F>
static inline TRT_HD trt_ds_pixel_out trt_ds_pixel(const trt_ds_args& a, const F& f, int x, int y, const float* color, const float* albedo, float depth,
                                                   float variance)
{
    trt_ds_pixel_out o;
    // steps 2, 4, 6 and 9: the input's bits
    o.color[0] = color[0];
    o.color[1] = color[1];
    o.color[2] = color[2];
    o.variance = variance;
    o.scale = 1.0f;
    if (!trt_dn_hit(depth)) return o;
    const float lp = trt_ds_luminance(color, albedo, depth);
    int n = 0;
    float s1 = 0.0f, s2 = 0.0f;
    bool flat = true;  // every counting tap carries l_p itself
    TRT_UNROLL
    for (int dy = -R; dy <= R; ++dy) {
        TRT_UNROLL
        for (int dx = -R; dx <= R; ++dx) {
            if (dx == 0 && dy == 0) continue;
            const float l = f(x + dx, y + dy);
            if (!trt_ds_finite(l)) continue;
            n = n + 1;
            s1 = s1 + l;
            s2 = s2 + l * l;
            flat = flat && l == lp;
        }
    }
    if (n < TRT_DS_MIN_TAPS) return o;
    // step 6 on a flat window, l_p = m = T: decided by comparison, since the rounded sum of n equal numbers over n may fall an ulp short of
    // them, and an emitter seen directly or a constant image would then be scaled by 1 - 2^-24 here and there
    if (flat) return o;
    const float fn = (float)n;
    const float m = s1 / fn;
    const float d = s2 / fn - m * m;
    const float v = d > 0.0f ? d : 0.0f;
    const float T = m + a.sigma * trt_sqrt(v);
    if (trt_ds_finite(lp) && trt_ds_finite(color[0]) && trt_ds_finite(color[1]) && trt_ds_finite(color[2])) {
        if (lp <= T) return o;
        if (lp > T) {  // step 7 (a T that is not a number is neither: the pixel passes through)
            const float s = T / lp;
            o.color[0] = color[0] * s;
            o.color[1] = color[1] * s;
            o.color[2] = color[2] * s;
            o.variance = (variance * s) * s;
            o.scale = s;
        }
        return o;
    }
    // step 8: a sample that is not a number is replaced by its surroundings' mean, before it can enter a history for good
    const trt_dn4 fa = trt_dn_factor(albedo[0], albedo[1], albedo[2]);
    o.color[0] = m * fa.x;
    o.color[1] = m * fa.y;
    o.color[2] = m * fa.z;
    o.variance = trt_ds_finite(variance) ? variance : 0.0f;
    o.scale = 0.0f;
    return o;
}

// This frame's pixels in row-major global memory: the fetch without a tile (TRT_DESPECKLE_LDS=0) and of the CPU build.
struct trt_ds_frame {
    const float* colorb;
    const float* albedob;
    const float* depthb;
    int width, height;
    TRT_HD float operator()(int x, int y) const
    {
        if (!trt_dn_inside(x, y, width, height)) return trt_ds_nan();
        const size_t q = (size_t)y * (size_t)width + (size_t)x;
        return trt_ds_luminance(colorb + 3 * q, albedob + 3 * q, depthb[q]);
    }
};

#endif  // TRT_DESPECKLE_H
