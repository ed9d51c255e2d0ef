/*
 * trt.h — C-ABI of the MI355X path-tracing hot path (libtrt_hip.so).
 *
 * This is the drop-in boundary for the per-pixel Monte-Carlo inner loop of
 * TinyRayTracing.  The reference has no FFI; its "render entry point" is the
 * body of main() (RayTracingOnCPU/main.cpp:79-113: the OpenMP sample/pixel
 * loop calling Camera::getRay camera.cpp:19-28, traverseBVH bvh.cpp:146-175
 * and shade pathTracing.cpp:3-102).  Every entry point below replaces a piece
 * of that loop; the citation says which.
 *
 * Plain C: pointers + sizes only, no C++/torch types.  All functions return 0
 * on success and a non-zero TRT_E* code on failure; the message is available
 * from trt_last_error() (thread-local).  The library never calls exit()
 * (the reference exit()s from its loaders, scene.cpp:10,64,122, and from
 * Sample(), pathTracing.cpp:129).
 */
#ifndef TRT_H
#define TRT_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRT_ABI_VERSION 5

/* error codes */
#define TRT_OK 0
#define TRT_EINVAL 1   /* bad argument / inconsistent scene */
#define TRT_EHIP 2     /* HIP runtime error */
#define TRT_ENOMEM 3   /* device or host allocation failed */
#define TRT_ENODEV 4   /* no usable gfx950 device */

/* Reference constants (pathtracing.h:11-12, bvh.h:5, ray.h:5-8, bvh.cpp:185,189). */
#define TRT_PI 3.1415926f
#define TRT_P_RR 0.8f
#define TRT_INF 114514.0f
#define TRT_T_MIN 0.0005f
#define TRT_PARALLEL_EPS 0.00001f
#define TRT_RAY_DIFFUSE 0
#define TRT_RAY_SPECULAR 1
#define TRT_RAY_TRANSMISSION 2
#define TRT_RAY_INVALID 3

/* ---- flat scene (what main.cpp hands the loop: scene.triangles in post-BVH
 *      order, scene.materials, scene.lights, scene.camera, root) ------------ */

/* BVH2 inner node, 64 B.  Replaces BVHNode (bvh.h:16-22: two pointers, index,
 * num, AA, BB).  The two children's padded boxes (bvh.cpp:31-40) live in the
 * parent so one 64-B fetch decides both descents (bvh.cpp:156-166).
 * child refs: bit31 = 0 -> index of an inner node;
 *             bit31 = 1 -> leaf: bits 30..27 = triangle count (0..15),
 *                                bits 26..0  = first triangle (post-BVH order).
 * Post-BVH order (what bvh.cpp's in-place sort leaves behind): every triangle under child0 has a lower index than
 * every triangle under child1; trt_create checks it (the tie rule of bvh.cpp:168-172 is applied by index).
 * Boxes: any finite coordinates or +-inf, nested or not (a subtree is entered iff the ray passes its stored box, bvh.cpp:162-166, whatever the boxes above
 * or below it say); a NaN coordinate is refused by trt_create (TRT_EINVAL): glm::min / glm::max pass a NaN on from their first operand only, so the reference's
 * own answer on such a box depends on the axis the NaN sits on.
 * Leaf size: any tree with leaves of 1..15 triangles is walked by the same kernels and gives the reference's hits on THAT tree.  As in the reference
 * (bvh.cpp:151-154) every triangle of a leaf is tested whenever the ray passes the leaf's box, so large leaves cost tests: the reference's own
 * buildBVH(..., 8) tree runs at about 0.8 of the speed of a tree built with 2 (every published number is on leaf 2). */
typedef struct trt_bvh_node {
    float lo0[3], hi0[3];
    float lo1[3], hi1[3];
    uint32_t child0, child1;
    uint32_t reserved[2];
} trt_bvh_node;

#define TRT_LEAF_BIT 0x80000000u
#define TRT_LEAF_COUNT(ref) (((ref) >> 27) & 15u)
#define TRT_LEAF_FIRST(ref) ((ref) & 0x07FFFFFFu)
#define TRT_MAKE_LEAF(first, count) (TRT_LEAF_BIT | ((uint32_t)(count) << 27) | (uint32_t)(first))
#define TRT_MAX_LEAF_TRIS 15u
#define TRT_MAX_TRIS 0x07FFFFFFu

/* Material (material.h:11-33) with the light's radiance folded in
 * (scene.cpp:50-52).  tex = -1 when map_Kd == "". */
typedef struct trt_material {
    float Kd[3], Ks[3], Tr[3];
    float Ns, Ni;
    float radiance[3];
    int32_t is_emissive;
    int32_t tex;
} trt_material;

/* One <light> element, XML order (scene.cpp:25-54).  area = Material::area
 * accumulated in readobj (scene.cpp:201-203).  `radiance` is kept for the caller's convenience only: both the emissive hit
 * (pathTracing.cpp:11) and the direct term (pathTracing.cpp:65) read materials[mat].radiance, and so does this library.
 * A scene may have 0 to TRT_MAX_SCENE_LIGHTS lights (trt_create refuses more with TRT_EINVAL).  Every light adds a 48-B shadow-ray
 * record per path to the queue memory of a pass (trt_params::mem_budget: 132 + 48 * n_lights bytes per path), 16 KiB of
 * counters per pass slot, and one shadow-ray launch per bounce.  With TRT_FLAG_ONE_LIGHT a render has one such record and one
 * such launch whatever the light count (132 + 48 bytes per path). */
#define TRT_MAX_SCENE_LIGHTS 65535u
typedef struct trt_light {
    int32_t mat;          /* material id of mtlname */
    float radiance[3];
    float area;           /* total area A_l of this light's triangles */
    uint32_t tri_first;   /* into light_tris */
    uint32_t tri_count;
} trt_light;

/* Copy of an emissive triangle kept per light material for sampling
 * (Material::triangles, scene.cpp:204); cum_area = Triangle::area, the
 * running total at the time it was appended (scene.cpp:203). */
typedef struct trt_light_tri {
    float v[3][3];
    float vn[3][3];
    float cum_area;
} trt_light_tri;

/* 8-bit RGB texture, row-major, row 0 first as stored in the file (the
 * reference indexes cv::Mat rows directly, pathTracing.cpp:22-25). */
typedef struct trt_texture {
    int32_t width, height;
    const uint8_t* rgb;
} trt_texture;

/* Camera after setCamera() (camera.cpp:3-17). */
typedef struct trt_camera {
    float eye[3];
    float lower_left_corner[3];
    float horizontal[3];
    float vertical[3];
} trt_camera;

typedef struct trt_scene {
    uint32_t n_tris;
    const float* tri_v;      /* [n_tris][3][3]  Triangle::v  (triangle.h:14), post-BVH order */
    const float* tri_vn;     /* [n_tris][3][3]  Triangle::vn (triangle.h:15) */
    const float* tri_vt;     /* [n_tris][3][2]  Triangle::vt (triangle.h:16) */
    const int32_t* tri_mat;  /* [n_tris] material id (replaces Triangle::mtl_name) */
    uint32_t n_nodes;
    const trt_bvh_node* nodes; /* nodes[0] is the root; n_nodes >= 1 */
    uint32_t bvh_depth;      /* max number of inner nodes on a root->leaf path */
    uint32_t n_materials;
    const trt_material* materials;
    uint32_t n_lights;       /* <= TRT_MAX_SCENE_LIGHTS (see trt_light) */
    const trt_light* lights;
    uint32_t n_light_tris;
    const trt_light_tri* light_tris;
    uint32_t n_textures;
    const trt_texture* textures;
    trt_camera camera;
} trt_scene;

/* ---- render parameters ---------------------------------------------------- */

#define TRT_FLAG_TIMING 1u   /* per-kernel hipEvent timing into trt_stats */
#define TRT_FLAG_COUNT 2u    /* count inner-node visits / triangle tests (stats kernels) */
#define TRT_FLAG_OVERLAP 4u  /* keep two sample passes in flight on two streams (+4-5 % throughput; per-kernel
                              * timings then include the other pass's kernels, so profiling runs leave it off) */
#define TRT_FLAG_FIXED_NEE 8u /* opt out of the reference's next-event-estimation quirks: every light's CDF
                              * draw spans that light's own area, light points are uniform on the chosen triangle, and the
                              * shadow test is an occlusion test up to the light sample (any hit in [0.0005, 0.999 * distance)
                              * blocks; a miss is visible) instead of closest-hit + material comparison; as everywhere, nothing farther than 114514 is seen (Q7).  Off = parity mode. */
#define TRT_FLAG_FIXED_PIXELS 16u /* opt out of the pixel-grid quirks (Q1, Q2): pixel (i, j) samples its own cell
                                  * [j/W, (j+1)/W) x [(H-1-i)/H, (H-i)/H) of the image plane uniformly.  Off = parity mode. */

#define TRT_FLAG_RAY_OFFSET 32u /* opt out of Q6 (rays start ON the surface they leave; only t < 0.0005, bvh.cpp:189, keeps them from
                                  * hitting it again, and at the 1000-unit distances of the Cornell box the hit point's rounding error
                                  * beats that for grazing directions): shadow and continuation rays start at P + s * eps * Ng, Ng the
                                  * hit triangle's geometric normal, s the side the ray leaves to, eps = 1e-4 * max(1, |P.x|, |P.y|, |P.z|).
                                  * Off = parity mode. */
#define TRT_OFFSET_EPS 0.0001f
#define TRT_FLAG_SPECULAR_KS 64u /* the look of the reference's own saved renders: the light that returns along a SPECULAR bounce is weighted by the material's Ks —
                                  * what the revision that wrote example-scenes-cg22/staircase/image*.png did — instead of the texel Kd the committed source
                                  * multiplies by (pathTracing.cpp:91-93, quirk Q8).  With it the HIP path reproduces staircase/image256.png to its noise floor
                                  * (profiles/r04_staircase_residual.txt); scenes whose glossy materials have Kd = Ks (veach-mis) or none (back) do not change.
                                  * Off = parity with the committed source. */
#define TRT_FLAG_ONE_LIGHT 128u /* stochastic light selection: every shaded path vertex samples ONE light, picked with probability proportional to its power, instead of
                                  * every light (pathTracing.cpp:34), and divides by that probability — unbiased, and a scene of any light count then has the shadow
                                  * rays, the launches and the path memory of a one-light scene.
                                  *   Needs TRT_FLAG_FIXED_NEE (rays aimed at different lights share one queue because the occlusion test needs no light material):
                                  *   TRT_FLAG_ONE_LIGHT without TRT_FLAG_FIXED_NEE is TRT_EINVAL, the handle stays usable.  Honoured by the entries that trace full
                                  *   paths (trt_render, _device, _samples, trt_render_pixels*, trt_render_rays*, trt_group_render*); the AOV and ray-query entries
                                  *   ignore it.  Off = every other mode, bit for bit.
                                  *   Weights: w_l = area_l * lum(radiance_l), lum = (0.2126 r + 0.7152 g) + 0.0722 b in fp32, radiance the light MATERIAL's;
                                  *   w_l = 0 unless area and luminance are both finite and > 0.  cdf_l = cdf_{l-1} + w_l in fp32, index order.
                                  *   Draw: one uniform u of the path's stream BEFORE the draws of the light sample; r = u * cdf_{L-1}; the pick is the first l with
                                  *   r < cdf_l (none by rounding: the last l with w_l > 0); the sample's contribution is multiplied by inv_p = cdf_{L-1} / w_l
                                  *   (one fp32 division, applied to the three components before the product with the path throughput).  cdf_{L-1} zero or not
                                  *   finite: the draw is spent, no light is sampled at the vertex.  The probability realised differs from w_l / sum(w) by the
                                  *   rounding of the fp32 prefix sums, about 1e-7 relative: that is the estimator's bias.
                                  *   Fewer than 2 lights: the flag does nothing, no draw is taken (TRT_FLAG_FIXED_NEE's render bit for bit).
                                  *   Path memory: 132 + 48 bytes per path and sample whatever the light count (trt_params::mem_budget).  trt_stats::rays_shadow
                                  *   counts what is traced: at most one ray per shaded vertex. */
#define TRT_FLAG_NEAR_LIGHTS 256u /* TRT_FLAG_ONE_LIGHT's one light picked where the vertex is: a stochastic descent of a binary tree over the lights, each child weighted
                                  * by its power over its squared distance from the vertex, the realised probability divided out — unbiased like TRT_FLAG_ONE_LIGHT,
                                  * with the same one queue, one shadow launch per bounce and 132 + 48 bytes per path.  Only the pick changes.
                                  *   Needs TRT_FLAG_ONE_LIGHT (and with it TRT_FLAG_FIXED_NEE): without it the call is TRT_EINVAL from the check that guards
                                  *   TRT_FLAG_ONE_LIGHT, the handle stays usable.  Honoured by the entries that honour TRT_FLAG_ONE_LIGHT (trt_render, _device, _samples,
                                  *   trt_render_pixels*, trt_render_rays*, trt_group_render*); the AOV and ray-query entries ignore it.  Off = every other mode, bit
                                  *   for bit.  Fewer than 2 lights: the flag does nothing, no draw is taken.
                                  *   Tree lights: light l is one if w_l > 0 (TRT_FLAG_ONE_LIGHT's weight), tri_count > 0 and every vertex of its light_tris is finite;
                                  *   M of them.  M == 0: no light is sampled at a vertex, no draw.  M == 1: that light, inv_p = 1, no draw.  M >= 2: the descent.
                                  *   Box of a light: the exact min and max over the vertices of its light_tris; its centre: 0.5f * lo + 0.5f * hi per axis.
                                  *   Tree (built on the host at trt_create whenever n_lights >= 2, deterministic): recurse on the list of tree lights, at first in
                                  *   index order.  One light: a leaf.  n >= 2: the axis of the largest extent (max - min, fp32) of the centres' bounds, ties to x,
                                  *   then y, then z; a stable sort by centre[axis]; the first floor(n / 2) lights go left, the rest right.  Nodes are numbered in
                                  *   pre-order (node, left subtree, right subtree): M - 1 nodes, depth <= ceil(log2 M) <= 16.  A node (64 bytes) holds per child c
                                  *   the box lo_c, hi_c of its lights, w_c = the fp32 sum of their weights in the child's list order (the order the split leaves,
                                  *   before the child sorts), and a reference: bit 31 set = leaf, low bits the light's index.
                                  *   Descent at P, the position of the path vertex, starting with inv_p = 1.  At each node, for each child c:
                                  *   centre = 0.5f * lo_c + 0.5f * hi_c, r2 = |hi_c - centre|^2, d2 = |P - centre|^2 (each (x*x + y*y) + z*z), m = fmaxf(d2, r2),
                                  *   imp_c = w_c / m.  s = imp0 + imp1; unless imp0 >= 0 && imp1 >= 0 && s > 0 && s < inf (a NaN fails it too) the node decides by
                                  *   power alone: imp_c = w_c, s = w0 + w1.  One uniform u of the path's stream, r = u * s; child 0 iff r < imp0; if the picked
                                  *   child's imp is not > 0, the other child.  inv_p = inv_p * (s / imp_picked).  Step into the picked child; stop at a leaf.
                                  *   All of it fp32, in this order, no contraction.  The draws — one per level — sit where TRT_FLAG_ONE_LIGHT's one draw sits, BEFORE
                                  *   the draws of the light sample, and the sample's contribution is multiplied by inv_p as under TRT_FLAG_ONE_LIGHT (the three
                                  *   components, before the product with the path throughput).  inv_p not finite at the leaf: the draws are spent, no light is
                                  *   sampled at the vertex.
                                  *   Every tree light has positive probability at every P (where one child's imp underflows to zero beside a positive one, that
                                  *   child's lights are the exception at that P), and the probability realised is 1 / inv_p up to the fp32 rounding of the
                                  *   products and quotients (about 2^-23 per level) and the 24-bit uniform per level: that is the estimator's bias.
                                  *   trt_update_geometry* with lights != NULL rebuilds the tree (and the weights) on the host from the new tables and uploads it:
                                  *   the handle then answers as a fresh one would.  With lights == NULL the tree is not touched, like the sampling tables.
                                  *   Memory: 64 bytes * (n_lights - 1) on the device for the nodes (M - 1 of them in use; an update may change M).  Path memory
                                  *   as under TRT_FLAG_ONE_LIGHT: 132 + 48 bytes per path and sample. */

typedef struct trt_params {
    int32_t width, height;   /* full image size (scene.img_width/height, scene.cpp:13-14) */
    int32_t spp;             /* SAMPLE (main.cpp:13,55) */
    uint32_t seed;           /* counter-RNG seed; stream = (seed, pixel y*width+x, sample) */
    /* tile rectangle [x0,x1) x [y0,y1) of the full image rendered by this call */
    int32_t x0, y0, x1, y1;
    /* row interleave for multi-GPU image tiling: only rows y (inside the tile)
     * with ((y / row_block) % row_mod) == row_rem are rendered; output rows are
     * packed in increasing y.  row_mod <= 1 renders every row. */
    int32_t row_block, row_mod, row_rem;
    int32_t max_depth;       /* 0 = unbounded like the reference (pathTracing.cpp:78-99) */
    uint32_t flags;
    uint64_t mem_budget;     /* bytes of HBM for path/queue state (132 + 48 * n_lights per path and sample in a pass; 132 + 48 under TRT_FLAG_ONE_LIGHT, whatever the light count); 0 = three quarters of
                              * what is free (one pass when it fits); too small for one sample of every pixel of the tile: TRT_ENOMEM */
} trt_params;

#define TRT_MAX_KERNELS 8
enum {
    TRT_K_GEN_PRIMARY = 0,  /* trt_render_rays*, trt_aov_rays*: the kernel that queues the caller's rays; 0 launches everywhere else (the camera's rays are generated inside bounce 0) */
    TRT_K_TRACE_CLOSEST = 1,
    TRT_K_SHADE = 2,
    TRT_K_TRACE_SHADOW = 3,
    TRT_K_RESOLVE = 4,
    TRT_K_TAIL = 5,       /* the last, short-queue bounces of a pass fused into one launch */
    TRT_K_DENOISE = 6,    /* trt_denoise*: the prepare kernel and every level of the a-trous filter; trt_reproject*: its one kernel (trt_reproject_moments*: its two); trt_despeckle*: its one kernel */
    TRT_K_REFIT = 7       /* trt_update_geometry*: every kernel of an update */
};

typedef struct trt_stats {
    uint64_t rays_camera;       /* primary rays traced */
    uint64_t rays_shadow;       /* NEE closest-hit rays traced (pathTracing.cpp:54) */
    uint64_t rays_indirect;     /* valid extension rays traced (pathTracing.cpp:81, INVALID excluded) */
    uint64_t shaded_hits;       /* path vertices that reached shade() */
    uint64_t inner_visits[2];   /* [closest, shadow] inner nodes visited = all child boxes fetched and tested (TRT_FLAG_COUNT);
                                 * inner_node_bytes says how much one visit reads */
    uint64_t tri_tests[2];      /* [closest, shadow] triangle tests (TRT_FLAG_COUNT) */
    uint64_t wave_steps[2];     /* wave-level iterations of the traversal kernels' [inner-node, leaf] phases (TRT_FLAG_COUNT):
                                 * inner_visits / (64 * wave_steps[0]) is the SIMD utilisation of the inner phase */
    uint64_t launches[TRT_MAX_KERNELS];
    double kernel_ms[TRT_MAX_KERNELS]; /* summed launch durations (TRT_FLAG_TIMING) */
    double render_ms;           /* first gen_primary launch -> last resolve, device time */
    uint32_t passes;            /* sample chunks the render was split into */
    uint32_t max_bounces;       /* deepest path vertex index reached */
    uint64_t rows_rendered;     /* rows in the packed output */
    uint32_t inner_node_bytes;  /* bytes one inner-node visit fetches: 64 (the caller's BVH2 node: two boxes + refs, tiny scenes),
                                 * 128 (its exact 4-wide collapse: four boxes + refs) or 80 (its 8-wide collapse with quantised boxes) */
    uint32_t redo_rays;         /* rays whose traversal result failed the check made when it is stored (a hit in front of the box of its
                                 * own leaf, or — 8-wide nodes — on a leaf whose exact box the ray misses), and rays with a direction component
                                 * of exactly zero (for them the reference's slab test can meet 0 * inf; they are traced with its literal form where
                                 * their origin may lie on a box plane), traced again in the exact form: a handful per 10^7, respectively one or two
                                 * per 10^5, on padded trees; a large number says the slow path is carrying the render */
    uint64_t lane_census[4];    /* TRT_FLAG_COUNT, persistent traversal kernels: summed over every wave iteration, the lanes waiting for a node
                                 * step [0], for a triangle step [1], holding a finished ray that waits for the refill batch [2]; [3] = the
                                 * iterations (x 64 = lane slots; what is left held no ray) — where the idle SIMD lanes are */
} trt_stats;

typedef struct trt_handle trt_handle;

/* Number of image rows a trt_params selects (tile rows passing the interleave). */
int trt_rows_selected(const trt_params* p);

/* Upload the flat scene to HBM on `device` (HIP ordinal) and build the
 * device-side 48-B Moller-Trumbore triangle records and 64-B shading records.
 * Replaces nothing the reference times; it is the hand-over of scene.triangles /
 * root to the loop at main.cpp:76-81. */
int trt_create(const trt_scene* scene, int device, trt_handle** out);

/* render(): replaces main.cpp:79-113.  Renders p->spp samples of every
 * selected pixel and writes the averaged linear radiance, RGB interleaved,
 * row-major, rows packed (see row_block), as float into a HOST buffer of
 * rows_selected * (x1-x0) * 3 floats.  `stats` may be NULL. */
int trt_render(trt_handle* h, const trt_params* p, float* out_rgb_host, trt_stats* stats);

/* Same, but out_rgb is DEVICE memory on the handle's device and all work is
 * enqueued on `hip_stream` (a hipStream_t, or NULL for the default stream);
 * returns after the stream has been synchronised. */
int trt_render_device(trt_handle* h, const trt_params* p, float* out_rgb_dev,
                      void* hip_stream, trt_stats* stats);

/* Progressive / resumable render.  The reference keeps one `double* image` for the whole run and adds
 * color/SAMPLE of every sample to it (main.cpp:74-75,101), then shows it once at the end (main.cpp:114).
 * This entry renders samples [sample_begin, sample_end) of the p->spp samples and adds them, in sample
 * order, onto `accum` — HOST, rows_selected * (x1-x0) * 3 doubles, in/out: the running sums of
 * (double)(L_s / spp).  Calls that cover [0, spp) in increasing order, starting from zeros, leave exactly
 * the sums of one trt_render call (and in out_rgb_host — optional, may be NULL — exactly its image), so
 * a long render can be shown while it converges, check-pointed (save accum + sample_end) and resumed.
 * A pixel whose camera rays provably miss the scene (trt_cull.h) is left alone instead of having +0.0
 * added to it per sample: the same value for every accum but one — a -0.0 handed in for such a pixel
 * stays -0.0 where the additions would have made it +0.0 (as they do with TRT_CULL_PRIMARY=0). */
int trt_render_samples(trt_handle* h, const trt_params* p, int32_t sample_begin, int32_t sample_end,
                       double* accum_host, float* out_rgb_host, trt_stats* stats);

/* Adaptive sampling: render samples [sample_begin, sample_end) of the LISTED pixels only.  pixels[i] = y * p->width + x
 * (< width * height), any order, duplicates allowed (every entry has its own slot).  For every entry i and every sample s, in
 * increasing s:
 *     v = (double)(L_s / (float)p->spp)             -- exactly the term trt_render_samples adds
 *     sum[3i + c]   += v_c
 *     sumsq[3i + c] += v_c * v_c                    -- a rounded double product, then a rounded double add (no fused multiply-add)
 * sum / sumsq: HOST, n_pixels * 3 doubles, in/out (sumsq may be NULL).  Sample s of pixel q is the path trt_render traces for it
 * (the random stream is keyed by (seed, q, s)), so a list holding every pixel of a tile in tile order, over [0, spp) from zeros,
 * leaves in sum exactly trt_render_samples' accum.  The tile and row-interleave fields of p are ignored; width, height, seed,
 * max_depth, flags and mem_budget mean what they mean for trt_render (mem_budget too small for one sample of every entry:
 * TRT_ENOMEM).  sample_end may exceed p->spp (p->spp is only the scale of v).  n_pixels == 0 or an empty range: nothing to do,
 * TRT_OK.  TRT_EINVAL: a null pointer while n_pixels > 0, an entry >= width * height, sample_begin < 0 or > sample_end, or
 * n_pixels > 0x7FFF0000 (the path ids of one pass).  stats: as for a render, with rows_rendered = 0. */
int trt_render_pixels(trt_handle* h, const trt_params* p, uint32_t n_pixels, const uint32_t* pixels,
                      int32_t sample_begin, int32_t sample_end, double* sum_host, double* sumsq_host, trt_stats* stats);
/* The same with pixels, sum and sumsq in DEVICE memory of the handle's device, all work on hip_stream (NULL = default);
 * returns after the stream has been synchronised. */
int trt_render_pixels_device(trt_handle* h, const trt_params* p, uint32_t n_pixels, const uint32_t* pixels_dev,
                             int32_t sample_begin, int32_t sample_end, double* sum_dev, double* sumsq_dev,
                             void* hip_stream, trt_stats* stats);

/* ---- full paths along rays the caller chose ----------------------------------------------------------------------------------
 * trt_render_rays is trt_render_pixels with the built-in ray generator replaced by the caller's arrays: n entries ("slots", each with its own
 * random stream and its own sums), samples [sample_begin, sample_end), one ray per entry and sample.  It serves a camera that moves while the
 * handle stays resident, any camera that is not the reference's pinhole (thin lens, fisheye, orthographic, stereo), and rays that start on
 * surfaces (light probes, irradiance samples, lightmap texels).  The handle keeps no state of it.
 *   Rays.  org / dir: [n_samples][n][3] floats, sample-major, n_samples = sample_end - sample_begin; the ray of (entry i, sample s) sits at
 *   index (s - sample_begin) * n + i.  stream[n] (uint32, may be NULL = i): the "pixel" word of the entry's random stream; any 32 bits.
 *   One path.  The path of (entry i, sample s) is exactly what trt_render traces from its bounce-0 ray on: the ray's type is camera, so a light
 *   hit directly is kept (pathTracing.cpp:9-12); depth 0, throughput 1; the random stream is (p->seed, stream[i], s), and THE FIRST DRAW INDEX
 *   IS 2: draws 0 and 1 of that stream belong to whoever generated the ray — the built-in camera spends them on its jitter (main.cpp:92-93),
 *   and a caller's generator may use them too (trt_prims.h trt_rng_uniform(key, 0 / 1)).
 *   Sums.  sum / sumsq: n * 3 doubles, in/out, the terms of trt_render_pixels in its order: v = (double)(L / (float)p->spp), sum += v,
 *   sumsq += v * v, in increasing s.  sumsq may be NULL.  sample_end may exceed p->spp (p->spp only scales v).
 *   The built-in camera.  trt_camera_rays(the handle's camera, p, pixels, ...) fed into trt_render_rays with stream = pixels leaves, bit for
 *   bit, what trt_render_pixels leaves for that pixel list — and with another trt_camera what a handle created with THAT camera would leave.
 *   Parameters.  max_depth, mem_budget (132 + 48 * n_lights bytes per path, as trt_render_pixels; TRT_ENOMEM when one sample of every entry
 *   does not fit) and the flags FIXED_NEE, RAY_OFFSET, SPECULAR_KS, TIMING, COUNT and OVERLAP mean what they mean for trt_render_pixels.
 *   trt_render_rays ignores width, height, the tile fields and TRT_FLAG_FIXED_PIXELS; trt_camera_rays honours width, height and
 *   TRT_FLAG_FIXED_PIXELS (and ignores the tile fields, spp, max_depth, mem_budget and every other flag).
 *   Directions are used as given.  Radiance is meaningful for unit directions only; a non-unit direction is not an error.
 *   Invalid entries.  An entry whose six components are not all finite (a NaN, an infinity), or whose direction is (0, 0, 0), is not traced:
 *   it adds exactly 0 to sum and sumsq for that sample, is not counted in stats.rays_camera, and never disturbs another entry.  A single zero
 *   component and denormals are valid.
 *   TRT_EINVAL, checked on the host before anything is written, the handle stays usable: a null handle or p; a null org, dir or sum while
 *   n > 0; n > 0x7FFF0000 (the path ids of one pass); sample_begin < 0 or > sample_end; p->spp < 1; max_depth < 0.  n == 0 or an empty sample
 *   range: nothing to do, TRT_OK.
 *   stats: as for trt_render_pixels; rays_camera counts the valid entries, rows_rendered = 0, and the kernels that bring the caller's rays into
 *   the queue are counted under TRT_K_GEN_PRIMARY.
 *   Cost.  Bounce 0 goes through HBM here (a 48-byte queue record written and read per path besides the 24 bytes of the ray) where the
 *   built-in camera forms its rays in registers; the host entry stages the rays pass by pass, never all at once. */
int trt_render_rays(trt_handle* h, const trt_params* p, uint32_t n, const float* org, const float* dir, const uint32_t* stream,
                    int32_t sample_begin, int32_t sample_end, double* sum_host, double* sumsq_host, trt_stats* stats);
/* The same with org, dir, stream, sum and sumsq in DEVICE memory of the handle's device, all work on hip_stream (NULL = default);
 * returns after the stream has been synchronised. */
int trt_render_rays_device(trt_handle* h, const trt_params* p, uint32_t n, const float* org_dev, const float* dir_dev, const uint32_t* stream_dev,
                           int32_t sample_begin, int32_t sample_end, double* sum_dev, double* sumsq_dev, void* hip_stream, trt_stats* stats);
/* The rays trt_render traces for the listed pixels (pixels[i] = y * p->width + x), samples [sample_begin, sample_end), of ANY camera: the
 * stream (p->seed, pixels[i], s), its draws 0 and 1 as the jitter, Camera::getRay (camera.cpp:19-28) — in the layout trt_render_rays reads,
 * org / dir [n_samples][n_pixels][3].  Host only: needs no handle and no GPU.  width and height >= 1 (a side of 1 gives what the reference's
 * x = j / (W - 1) gives: NaN, unless TRT_FLAG_FIXED_PIXELS).  TRT_EINVAL, before anything is written: a null cam or p, a null array while
 * n_pixels > 0, width or height < 1, width * height > 2^32 (a pixel is a 32-bit index), sample_begin < 0 or > sample_end, an entry >= width * height. */
int trt_camera_rays(const trt_camera* cam, const trt_params* p, uint32_t n_pixels, const uint32_t* pixels,
                    int32_t sample_begin, int32_t sample_end, float* org_host, float* dir_host);
/* The same bits on `device` (HIP ordinal; a gfx950, else TRT_ENODEV) with pixels, org and dir in DEVICE memory, the work on hip_stream
 * (NULL = default); returns after the stream has been synchronised.  An entry >= width * height is found by the kernel: TRT_EINVAL after
 * the fact, with org / dir written for the other entries.  A few bytes of device memory are allocated and freed per call. */
int trt_camera_rays_device(int device, const trt_camera* cam, const trt_params* p, uint32_t n_pixels, const uint32_t* pixels_dev,
                           int32_t sample_begin, int32_t sample_end, float* org_dev, float* dir_dev, void* hip_stream);

/* First-hit feature buffers ("AOVs") for denoisers: per-pixel albedo, shading normal and depth, the inputs OIDN / OptiX / SVGF-style
 * filters take beside a low-spp render.  For every selected pixel (x, y) of the tile (tile and row interleave exactly as trt_render)
 * and every sample s in [0, p->spp):
 *   - the camera ray trt_render traces for (pixel y * width + x, sample s): same random stream, same jitter, TRT_FLAG_FIXED_PIXELS honoured;
 *   - its closest hit (t, tri, u, v) as trt_render's bounce 0 and trt_trace_closest define it;
 *   - a hit, on any material (emissive ones included): albedo = the texel or Kd that shade() weights by (pathTracing.cpp:15-30, nearest
 *     texel), normal = the normalised interpolated vertex normal (bvh.cpp:223-224), depth = t;
 *     a miss: albedo = normal = (0, 0, 0), depth = TRT_INF;
 *   - per channel v = value / (float)p->spp (a float division, as trt_render's resolve makes it), added as (double)v in increasing s onto a
 *     per-pixel double sum; the output is (float)sum.
 * So a call with spp = S gives the mean over the primary hits of samples 0..S-1 of any render with the same seed and flags: the beauty may
 * be rendered at 1024 spp and the AOVs at 16.  The normal is a mean of unit vectors and is NOT renormalised (it is shorter than 1 where
 * the samples of a pixel hit differently oriented surfaces, and (0, 0, 0) where they all miss).
 * Flags other than TRT_FLAG_FIXED_PIXELS, TRT_FLAG_TIMING and TRT_FLAG_COUNT, and max_depth, do not change the result (TRT_FLAG_OVERLAP
 * is ignored).  Buffers (HOST): albedo and normal rows_selected * (x1-x0) * 3 floats, RGB / XYZ interleaved, rows packed as in
 * trt_render; depth rows_selected * (x1-x0) floats.  Any of the three may be NULL, not all three (TRT_EINVAL).  Parameters are checked
 * as for trt_render.  mem_budget counts this call's path state, 20 bytes per path and sample in a pass (TRT_ENOMEM when one sample of
 * every pixel does not fit).  stats: rays_camera = paths traced; the traversal under TRT_K_TRACE_CLOSEST, the per-pixel accumulation under
 * TRT_K_RESOLVE; passes, rows_rendered, redo_rays and the TRT_FLAG_COUNT counters as for a render. */
int trt_render_aov(trt_handle* h, const trt_params* p, float* albedo_host, float* normal_host, float* depth_host, trt_stats* stats);
/* The same with the three buffers in DEVICE memory of the handle's device, all work on hip_stream (NULL = default stream); returns
 * after the stream has been synchronised. */
int trt_render_aov_device(trt_handle* h, const trt_params* p, float* albedo_dev, float* normal_dev, float* depth_dev,
                          void* hip_stream, trt_stats* stats);

/* ---- first-hit feature buffers along rays the caller chose ---------------------------------------------------------------------
 * trt_aov_rays is trt_render_aov with the built-in ray generator replaced by the caller's arrays, as trt_render_rays is to trt_render_pixels:
 * the albedo, normal and depth of a camera that moves while the handle stays resident, of a thin lens, a fisheye, or of probe rays.  The
 * handle keeps no state of it.
 *   Rays.  Exactly trt_render_rays' arrays: org / dir [n_samples][n][3] floats, sample-major, n_samples = sample_end - sample_begin; the ray of
 *   (entry i, sample s) sits at index (s - sample_begin) * n + i.  There are no stream ids: a first hit draws nothing.
 *   Per ray.  The closest hit (t, tri, u, v) as trt_trace_closest defines it (the same leaf-box rule, the same tie rules, bound TRT_INF), then
 *   the features as trt_render_aov defines them: a hit, on any material, gives albedo = the texel or Kd, normal = the normalised interpolated
 *   vertex normal, depth = t — in units of the direction's length: directions are used as given; a miss gives (0, 0, 0), (0, 0, 0), TRT_INF.
 *   Invalid entries.  An entry whose six components are not all finite, or whose direction is (0, 0, 0) (trt_render_rays' rule), counts as a
 *   MISS for that sample, is not counted in stats.rays_camera and never disturbs another entry.  It is not traced as given: a fixed finite
 *   ray takes its place in the queue and its record is marked, so no result depends on what a walk does with a NaN.  A single zero
 *   component and denormals are valid.
 *   Sums.  albedo_sum[3n], normal_sum[3n], depth_sum[n] doubles, in/out: per channel v = value / (float)p->spp (a float division), and
 *   sum += (double)v in increasing s.  Nothing is zeroed and nothing is rounded to float.  Any of the three may be NULL, not all three.
 *   sample_end may exceed p->spp (p->spp only scales v).
 *   The built-in camera.  With the rays of trt_camera_rays(the handle's camera, p, the pixels of a tile in tile order, 0, p->spp) and sums
 *   that start at zero, (float)sum is trt_render_aov's output for that tile, bit for bit — and with another trt_camera it is what a handle
 *   created with THAT camera would return.
 *   Parameters.  spp (the scale), mem_budget, TRT_FLAG_TIMING and TRT_FLAG_COUNT are honoured; width, height, the tile fields, seed,
 *   max_depth and every other flag are ignored.  mem_budget counts this call's path state, TRT_AOV_RAYS_BYTES_PER_PATH = 52 bytes per path
 *   and sample in a pass (a 32-byte packed ray, a 16-byte hit record, a 4-byte entry of the redo list); 0 = three quarters of what is free;
 *   TRT_ENOMEM when one sample of every entry does not fit.  The host entry stages the rays pass by pass, never all at once (24 bytes per
 *   path of a pass, beside the budget) and keeps a device copy of the given sums for the call.
 *   TRT_EINVAL, checked on the host before anything is written, the handle stays usable: a null handle or p; a null org or dir while n > 0;
 *   all three sums null; n > 0x7FFF0000; sample_begin < 0 or > sample_end; p->spp < 1.  Otherwise n == 0 or an empty sample range: nothing
 *   to do, TRT_OK.
 *   stats: rays_camera = the valid entries traced; the packing under TRT_K_GEN_PRIMARY, the traversal under TRT_K_TRACE_CLOSEST, the
 *   accumulation under TRT_K_RESOLVE, one launch of each per pass; passes, redo_rays and the TRT_FLAG_COUNT counters as for trt_render_aov
 *   (a placeholder ray is walked and counted like any ray that misses the root); rows_rendered = 0.
 *   Cost.  Every ray goes through HBM three times here (24 bytes read and a 32-byte record written by the packing, the record read by the
 *   traversal) where trt_render_aov forms its rays in registers.  Not yet measured on a GPU against trt_render_aov_device
 *   (tools/aov_rays_cost.py measures it; profiles/aov_rays_cost.txt will hold the figures). */
#define TRT_AOV_RAYS_BYTES_PER_PATH 52u
int trt_aov_rays(trt_handle* h, const trt_params* p, uint32_t n, const float* org, const float* dir, int32_t sample_begin, int32_t sample_end,
                 double* albedo_sum_host, double* normal_sum_host, double* depth_sum_host, trt_stats* stats);
/* The same with org, dir and the three sums in DEVICE memory of the handle's device (the sums are added onto in place), all work on hip_stream
 * (NULL = default); returns after the stream has been synchronised. */
int trt_aov_rays_device(trt_handle* h, const trt_params* p, uint32_t n, const float* org_dev, const float* dir_dev, int32_t sample_begin,
                        int32_t sample_end, double* albedo_sum_dev, double* normal_sum_dev, double* depth_sum_dev, void* hip_stream, trt_stats* stats);

/* traverseBVH (bvh.cpp:146-175) on a batch of n rays given as HOST arrays
 * org[n][3], dir[n][3].  Outputs (host): t[n] (TRT_INF on miss), tri[n]
 * (post-BVH triangle index, -1 on miss), uv[n][2] (barycentrics of v1,v2).
 * `stats` (optional) receives inner_visits[0]/tri_tests[0] and kernel_ms.
 * One rule beyond bvh.cpp's text ("Formulation"): a triangle hit whose distance lies IN FRONT of the box of the
 * leaf the triangle sits in — by more than a tolerance of 2^-16 relative plus 2^-17 of the scene's largest coordinate — does
 * not count: for a ray within ~1e-4 rad of a triangle's plane the computed distance can come out there; the reference rejects
 * such hits through its inside test on the computed point (bvh.cpp:191-198).  The tolerance keeps the rule off honest hits:
 * leaf boxes need NOT be padded (a triangle lying on a face of its leaf's box is found), at any coordinate magnitude. */
int trt_trace_closest(trt_handle* h, uint64_t n, const float* org, const float* dir,
                      float* t, int32_t* tri, float* uv, trt_stats* stats);

/* Ray queries with a per-ray search range.  t_max[n] (may be NULL: TRT_INF for every ray) bounds each ray: a hit counts iff
 * TRT_T_MIN <= t < bound (strict), bound = t_max > TRT_T_MIN ? fminf(t_max, TRT_INF) : TRT_T_MIN — so NaN, negative values, 0 and
 * TRT_T_MIN find nothing, and +inf or anything beyond TRT_INF is TRT_INF (Q7).  t_min stays the reference's 0.0005.  Whether a hit is
 * accepted (the leaf-box rule above, the emissive tie rules) does not depend on the bound: at equal t every tied candidate lies on the same
 * side of it.  Arguments are checked as for trt_trace_closest: a null handle or array (uv and t_max excepted) or n > 0x7FFF0000 is
 * TRT_EINVAL, n == 0 is TRT_OK.
 *
 * trt_trace_closest_range: the record trt_trace_closest returns when that hit lies inside the bound, otherwise exactly its miss record
 * (t = TRT_INF, not the bound; tri = -1; uv = (0, 0)).  uv may be NULL.  With t_max NULL it IS trt_trace_closest.  stats: the slots
 * trt_trace_closest fills (inner_visits[0], tri_tests[0], launches / kernel_ms[TRT_K_TRACE_CLOSEST], redo_rays). */
int trt_trace_closest_range(trt_handle* h, uint64_t n, const float* org, const float* dir, const float* t_max,
                            float* t, int32_t* tri, float* uv, trt_stats* stats);
/* The same with org, dir, t_max, t, tri and uv in DEVICE memory of the handle's device; all work on hip_stream (NULL = default stream), and
 * the call returns after that stream has been synchronised.  Nothing but the stats crosses PCIe. */
int trt_trace_closest_device(trt_handle* h, uint64_t n, const float* org, const float* dir, const float* t_max,
                             float* t, int32_t* tri, float* uv, void* hip_stream, trt_stats* stats);
/* Occlusion ("is anything between here and there?"): occluded[i] = 1 iff some hit counts for ray i, else 0 — one byte per ray.  The walk
 * stops at the first leaf that yields an accepted hit (no closest hit is searched for, no hit record is written), so it costs at most what
 * trt_trace_closest_range costs on the same rays.  stats: the shadow slots — inner_visits[1], tri_tests[1], launches /
 * kernel_ms[TRT_K_TRACE_SHADOW], rays_shadow = n — and redo_rays. */
int trt_trace_occluded(trt_handle* h, uint64_t n, const float* org, const float* dir, const float* t_max,
                       uint8_t* occluded, trt_stats* stats);
/* The same with org, dir, t_max and occluded in DEVICE memory, as trt_trace_closest_device. */
int trt_trace_occluded_device(trt_handle* h, uint64_t n, const float* org, const float* dir, const float* t_max,
                              uint8_t* occluded, void* hip_stream, trt_stats* stats);

/* Where is, or was, the surface a ray sees on OTHER vertex positions?  Per ray the closest hit (tri, u, v) exactly as trt_trace_closest
 * defines it on the handle's CURRENT geometry (the same leaf-box rule, the same tie rules, bound TRT_INF, the same redo path); then with
 * a, b, c = tri_v_other[tri][0..2] and w = (1.0f - u) - v:  point_k = (w * a_k + u * b_k) + v * c_k, fp32 in this order, no contraction
 * (hitPoint, tinyraytracing_amd/csrc/trt_path.h: a CPU build gives the same bits).  A miss writes three quiet NaNs (bits 0x7FC00000).
 * tri_v_other: [n_tris][3][3] in post-BVH order, the layout of trt_scene::tri_v and trt_geometry_update::tri_v — e.g. the vertices the handle
 * had before trt_update_geometry, which makes `point` the previous world position of what each ray sees now: the motion vectors
 * trt_reproject_motion needs.  With the handle's own vertices it is the hit point itself.  org, dir [n][3], point [n][3]: HOST arrays;
 * tri_v_other is staged in device memory for the call.  TRT_EINVAL, before any device work: a null argument; n_tris other than the
 * handle's; n > 0x7FFF0000.  n == 0 is TRT_OK.  Per ray 12 bytes are written: no t, tri or uv arrays.  stats: trt_trace_closest's slots. */
int trt_trace_points(trt_handle* h, uint64_t n, const float* org, const float* dir, const float* tri_v_other, uint32_t n_tris,
                     float* point, trt_stats* stats);
/* The same with org, dir, tri_v_other and point in DEVICE memory of the handle's device, as trt_trace_closest_device. */
int trt_trace_points_device(trt_handle* h, uint64_t n, const float* org, const float* dir, const float* tri_v_other, uint32_t n_tris,
                            float* point, void* hip_stream, trt_stats* stats);

void trt_destroy(trt_handle* h);

/* ---- geometry that moves: keep the tree, recompute its boxes ("refit") ----------------------------------------------------------
 * trt_update_geometry gives the triangles of a handle new coordinates.  Topology, triangle order, materials, texture coordinates, textures,
 * camera and every tuning decision of trt_create (trace_impl, the k_shade tables, slim / binned walk, grids, spill sizes) stay; only
 * coordinates change.  The cost is a pass over the triangles and the nodes on the device instead of trt_create's host work.
 *   Boxes.  A leaf's box becomes, per axis, min(coordinates of its triangles) - 0.001f / max + 0.001f (what the reference pads every node by,
 *   bvh.cpp:31-40, and what the builders of this repository emit); an inner child's box becomes the union of that child's two boxes.  Both are
 *   exact in fp32 (min / max and one rounded add; rounding is monotone, so the union of padded boxes is the padded union).  A leaf of 0 triangles
 *   keeps the box it has; so does a node no root path reaches.
 *   Result.  After the call the handle answers every entry point exactly as a fresh handle would that was created from the same trt_scene with
 *   tri_v (tri_vn, lights, light_tris) replaced and `nodes` carrying the boxes above — bit for bit: hits depend on the tree only through the
 *   stored boxes and the leaf order (trt_bvh_node above), refit boxes nest, and every node kind gives the same results.  All derived device
 *   state follows: the intersection and shading records (geometry rewritten, material and flags kept), the caller's nodes, the per-triangle leaf
 *   boxes, the 4-wide nodes and, on a handle that walks them, the 8-wide compressed nodes with their triangle records (each refitted
 *   in its own tree: the collapses chosen at trt_create only dropped boxes and stay valid; the 8-wide bytes come from the quantiser trt_create
 *   uses, so a stored box contains the exact one), the box-plane filter, the leaf-box tolerance, the light boxes, and the tables k_shade stages.
 *   A handle that walks the 8-wide nodes and whose new boxes reach 2^40 (the premise of that node kind) walks the exact 4-wide nodes from then
 *   on, for good; results do not change (trt_stats::inner_node_bytes then says 128).  A tree whose boxes did not nest at trt_create nests
 *   afterwards but stays without distance culling (correct, slower).
 *   Lights.  lights / light_tris (both or neither, HOST memory in both entries) replace the sampling tables; counts, every light's material and
 *   the ranges must fit the handle's (TRT_EINVAL otherwise).  A handle that bisects the packed CDF (every handle whose CDFs were non-decreasing
 *   at trt_create) refuses tables whose cumulative areas decrease or are NaN with TRT_EINVAL; one that scans keeps scanning.  With lights NULL
 *   the tables are not touched: correct iff no emissive triangle moved — the library does not check.  The light boxes are recomputed either way.
 *   Checks, all before anything is written: a null handle, u or tri_v, n_tris other than the handle's, the light checks above -> TRT_EINVAL on
 *   the host; a vertex coordinate that is NaN or infinite -> TRT_EINVAL from a reduction over the new vertices that runs first.  After any
 *   TRT_EINVAL the handle is unchanged and usable.  Normals may hold anything, as at trt_create.
 *   Calls on one handle are the caller's to serialise.  Both entries return after the stream has been synchronised.  Device memory: the first
 *   update allocates one 4-byte index per BVH2 node and per 4-wide node, and 28 bytes per 8-wide node (index + the exact union of its slots) on
 *   a handle that walks them (about 5 bytes per triangle on a leaf-2 tree, 16 at most), plus a few words per light and material, kept until trt_destroy; a handle that is never updated costs nothing.  The host entry also stages the
 *   vertices (36 bytes per triangle, 72 with normals) for the duration of the call.
 *   stats (optional): launches / kernel_ms[TRT_K_REFIT] = every kernel of the update, render_ms = the call's device time (copies included);
 *   every other field 0.  trt_group handles are not updated (re-create the group). */
typedef struct trt_geometry_update {
    const float* tri_v;               /* [n_tris][3][3], post-BVH order as in trt_scene; required */
    const float* tri_vn;              /* [n_tris][3][3] or NULL = normals stay */
    const trt_light* lights;          /* HOST in both entries; NULL = light tables stay */
    const trt_light_tri* light_tris;  /* HOST in both entries; NULL iff lights is NULL */
    uint32_t n_lights, n_light_tris;  /* must equal the handle's when lights != NULL */
} trt_geometry_update;
int trt_update_geometry(trt_handle* h, const trt_geometry_update* u, uint32_t n_tris, trt_stats* stats);
/* The same with tri_v / tri_vn in DEVICE memory of the handle's device, all work on hip_stream (NULL = default stream). */
int trt_update_geometry_device(trt_handle* h, const trt_geometry_update* u, uint32_t n_tris, void* hip_stream, trt_stats* stats);

/* ---- denoising: the edge-avoiding a-trous wavelet filter (Dammertz et al. 2010, the spatial part of SVGF) ------------------------
 * A feature-guided spatial filter of one W x H image.  It needs no scene handle: any image with these buffers can be filtered, one read
 * from PFM files included.  Inputs (all float, rows top to bottom, row-major):
 *   color     W*H*3  linear RGB;
 *   variance  W*H    the variance of the pixel's MEAN luminance, luminance = Rec. 709 (0.2126, 0.7152, 0.0722);
 *   albedo    W*H*3  and normal W*H*3 as trt_render_aov defines them (normals need not be unit length);
 *   depth     W*H    >= TRT_INF means a miss.
 * A pixel is a HIT iff depth < TRT_INF.  Taps outside the image are skipped (no clamping, no mirroring).  h = {1/16, 1/4, 3/8, 1/4, 1/16}.
 *  1. Demodulate: a_c = albedo_c > 0 ? albedo_c : 1;  c = color / a;  var = variance / max(lum(a), 1e-6)^2.
 *  2. Depth gradient, once: per axis the smaller |z_q - z_p| over the two axis neighbours q that are in-image hits (0 if there is none);
 *     gz = max(axis_x, axis_y).
 *  3. Levels k = 0 .. iterations-1, step s = 2^k; a miss pixel passes through unchanged, and for a hit pixel p:
 *     sd_p = sqrt(G3(var)_p), G3 = the 3x3 binomial [1/4, 1/2, 1/4]^2 over the in-image taps, renormalised;
 *     every tap q = p + s (i-2, j-2), j outer, i inner, that is in the image and a hit gets w = h_i h_j wn wz wl with
 *       wn = max(0, n_p . n_q)^sigma_normal           (an integer power, by repeated squaring: 128 is 7 squarings),
 *       wz = exp(-|z_p - z_q| / (sigma_depth gz_p |q - p| + 1e-3 z_p))   (|q - p| the Euclidean pixel distance),
 *       wl = exp(-|l_p - l_q| / (sigma_luminance sd_p + 1e-6))            (l = lum(c));
 *     the centre tap has w = (3/8)^2 (its feature weights are 1 by definition);
 *     c'_p = sum w c_q / sum w,  var'_p = sum w^2 var_q / (sum w)^2.
 *  4. Remodulate: out = c a (every pixel).
 * Arithmetic: fp32 throughout, exponentials by trt_expf_neg (include/trt_prims.h); the exact operation order is
 * tinyraytracing_amd/csrc/trt_denoise.h, which a CPU build of the same code reproduces bit for bit.  Non-finite colour or variance is
 * the caller's business: the result near such pixels is unspecified, but the call does not fault.
 * Costs: 64 bytes of device scratch per pixel (plus 56 for the staging of the host entry), allocated per call and freed before it returns. */
typedef struct trt_denoise_params {
    int32_t iterations;      /* levels, 1..10; 0 = 5 */
    int32_t sigma_normal;    /* the normal weight's exponent, 1..256; 0 = 128 */
    float sigma_depth;       /* >= 0; 0 = 1 */
    float sigma_luminance;   /* >= 0; 0 = 4 */
    uint32_t flags;          /* reserved, 0 */
} trt_denoise_params;
#define TRT_DENOISE_MAX_ITERATIONS 10
#define TRT_DENOISE_MAX_PIXELS (1u << 28)

/* Filters HOST buffers (out: W*H*3 floats) on `device` (HIP ordinal; a gfx950, else TRT_ENODEV).  params may be NULL (every default).
 * TRT_EINVAL: a null buffer, width or height < 1, width * height > TRT_DENOISE_MAX_PIXELS, iterations outside 0..10, sigma_normal outside
 * 0..256, a negative or NaN sigma, nonzero flags.  stats (optional): launches / kernel_ms[TRT_K_DENOISE] = the filter's kernels,
 * render_ms = the call's device time (copies included); every other field 0. */
int trt_denoise(int device, const trt_denoise_params* params, int width, int height, const float* color, const float* variance,
                const float* albedo, const float* normal, const float* depth, float* out, trt_stats* stats);
/* The same with every buffer in DEVICE memory of `device`, the work enqueued on hip_stream (NULL = default stream); returns after that
 * stream has been synchronised.  Nothing but the stats crosses PCIe; out is written at its first W*H*3 floats only. */
int trt_denoise_device(int device, const trt_denoise_params* params, int width, int height, const float* color, const float* variance,
                       const float* albedo, const float* normal, const float* depth, float* out, void* hip_stream, trt_stats* stats);

/* ---- temporal accumulation: reproject the previous frame's history (the temporal half of SVGF) --------------------------------------
 * A stateless image-space operation shaped like trt_denoise: one W x H image, no scene handle, no state in the library.  The caller owns
 * the history and hands it back frame after frame; what comes out goes on to trt_denoise.  All buffers float, rows top to bottom.
 * Inputs of the current frame, exactly trt_denoise's five: color W*H*3, variance W*H, albedo W*H*3, normal W*H*3, depth W*H.
 * History, all four or none (all NULL = a first frame):
 *   prev_cv      W*H*4  demodulated colour and its variance, the cv record (c.r, c.g, c.b, var) of trt_denoise.h (an earlier call's out_cv);
 *   prev_len     W*H    history length (an earlier call's out_len);
 *   prev_normal  W*H*3  and prev_depth W*H: the previous frame's own feature buffers.
 * Outputs, none of which may alias an input (not checked):
 *   out_color W*H*3 and out_variance W*H   what the caller hands to trt_denoise in place of color and variance;
 *   out_cv W*H*4 and out_len W*H           the next frame's history, together with this frame's normal and depth.
 * Per pixel p = (x, y):
 *  1. Demodulate as trt_denoise does (the same functions: history and filter share one domain): a_c = albedo_c > 0 ? albedo_c : 1,
 *     c = color / a, var = variance / max(lum(a), 1e-6)^2.
 *  2. A pixel with no history — a miss (depth >= TRT_INF, or a NaN), or any pixel when the history is NULL — gives out_color and
 *     out_variance = the input's bits, out_cv = (c, var), out_len = 1.
 *  3. World point P = cur.eye + depth d, d the unit direction through the pixel's centre: d = normalize(llc + s horizontal + t vertical - eye)
 *     with, under TRT_FLAG_FIXED_PIXELS, s = (x + 0.5) / W, t = (H - 1 - y + 0.5) / H, otherwise the reference's grid (quirks Q1, Q2 with
 *     both jitters at 0.5): s = x / (W - 1), t = (H - y) / (H - 1).  fp32 throughout (a render's binary64 grid is not needed here).
 *  4. Into the previous image: P - prev.eye = k ((prev.llc - prev.eye) + s' prev.horizontal + t' prev.vertical), solved by Cramer's rule;
 *     a zero determinant, k <= 0 or anything that is not a number: no history.  (s', t') gives continuous pixel coordinates (fx, fy) by the
 *     inverse of the grid of step 3, and z' = |P - prev.eye| is the depth the previous frame would have stored.  If cur and prev are
 *     byte-identical the geometry is skipped: fx = x, fy = y, z' = depth, so a still camera accumulates without resampling blur.
 *  5. Taps: the four pixels around (fx, fy), x0 = floor(fx), y0 = floor(fy), in the order (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1), with
 *     their bilinear weights.  (fx, fy) outside (-1, W) x (-1, H): no history.  A tap q counts iff its weight is > 0, it is inside the
 *     image, prev_depth_q < TRT_INF, |z' - prev_depth_q| <= depth_tolerance z', and n_p . n_q > 0 with
 *     (n_p . n_q)^2 >= normal_threshold^2 |n_p|^2 |n_q|^2 (normals are means of unit vectors, not unit: this form needs no square root).
 *     W_s = the sum of the weights of the counting taps; W_s < 0.01: no history.  Otherwise c_h, var_h and N_h are the weighted means of
 *     prev_cv and prev_len over the counting taps.
 *  6. Blend: N = min(N_h + 1, max_history), alpha' = max(alpha, 1 / N); c' = c_h + alpha' (c - c_h); var' = alpha'^2 var + (1 - alpha')^2 var_h;
 *     out_cv = (c', var'), out_len = N, out_color = c' a, out_variance = var' max(lum(a), 1e-6)^2.  So the history is the running mean of the
 *     frames until 1 / N falls below alpha, and an exponential average from then on.
 *  7. A hit pixel that found no history gives the results of step 2.
 * The variance formula takes the frames as independent estimates: the caller MUST change the seed every frame.
 * Geometry that moved between the frames (trt_update_geometry) is not tracked by THIS entry: the history of such a surface is used whenever
 * it passes the tests of step 5.  trt_reproject_motion below takes each pixel's previous world point (trt_trace_points) and follows it.
 * Arithmetic: fp32 throughout, the two normalisations by trt_sqrt (include/trt_exact.h); the exact operation order is
 * tinyraytracing_amd/csrc/trt_reproject.h, which a CPU build of the same code reproduces bit for bit.  Non-finite colours are the caller's
 * business, as for trt_denoise: no fault, the result is unspecified nearby.  Non-finite depths or camera values index nothing out of bounds:
 * such a pixel has no history. */
typedef struct trt_reproject_params {
    trt_camera cur, prev;     /* the cameras of this frame and of the history */
    float alpha;              /* least weight of the new frame, (0, 1]; 0 = 0.2 */
    float depth_tolerance;    /* relative, >= 0; 0 = 0.1 */
    float normal_threshold;   /* cosine, [0, 1]; 0 = 0.9 */
    float max_history;        /* cap of the history length, >= 1; 0 = 255 */
    uint32_t flags;           /* TRT_FLAG_FIXED_PIXELS only: which pixel grid the cameras use; any other bit TRT_EINVAL */
} trt_reproject_params;

/* Reprojects HOST buffers on `device` (HIP ordinal; a gfx950, else TRT_ENODEV); the buffers are staged in device memory for the call (80
 * bytes per pixel, 116 with a history).  TRT_EINVAL, checked in this order before any device work: null params or a null required buffer
 * (the five inputs, the four outputs); a history given in part; width or height < 1; width * height > TRT_DENOISE_MAX_PIXELS; alpha outside
 * [0, 1] or NaN; a negative or NaN depth_tolerance; normal_threshold outside [0, 1]; max_history neither 0 nor >= 1; a flag other than
 * TRT_FLAG_FIXED_PIXELS.  stats (optional): launches / kernel_ms[TRT_K_DENOISE] = the one kernel, render_ms = the call's device time (copies
 * included); every other field 0. */
int trt_reproject(int device, const trt_reproject_params* params, int width, int height, const float* color, const float* variance,
                  const float* albedo, const float* normal, const float* depth, const float* prev_cv, const float* prev_len,
                  const float* prev_normal, const float* prev_depth, float* out_color, float* out_variance, float* out_cv, float* out_len,
                  trt_stats* stats);
/* The same with every buffer in DEVICE memory of `device`, the work enqueued on hip_stream (NULL = default stream); returns after that
 * stream has been synchronised.  Nothing but the stats crosses PCIe and no device memory is allocated.  prev_cv and out_cv are read and
 * written as 16-byte records: an address that is not a multiple of 16 is TRT_EINVAL. */
int trt_reproject_device(int device, const trt_reproject_params* params, int width, int height, const float* color, const float* variance,
                         const float* albedo, const float* normal, const float* depth, const float* prev_cv, const float* prev_len,
                         const float* prev_normal, const float* prev_depth, float* out_color, float* out_variance, float* out_cv,
                         float* out_len, void* hip_stream, trt_stats* stats);

/* trt_reproject for surfaces that move.  One more required input, prev_point W*H*3: the world position, at the time of the history frame,
 * of the surface seen through each pixel now — trt_trace_points along the rays through the pixel centres of `cur`, on the vertices the
 * geometry had when the history frame was rendered.  The contract is trt_reproject's with steps 3 and 4 replaced:
 *  3'. v = prev_point - prev.eye.  (`cur` is not used.)
 *  4'. (k, s', t') from v by the same Cramer's rule, (fx, fy) by the same inverse grid, z' = |v| (trt_sqrt).  A zero determinant, k <= 0 (a
 *      point behind or on the previous eye), a point that is not a number (a miss of trt_trace_points) or a z' that is not finite: no
 *      history.  The shortcut for byte-identical cameras is NOT taken: a still camera does not mean a still surface.
 * Steps 1, 2, 5, 6 and 7 are trt_reproject's, through the same functions (tinyraytracing_amd/csrc/trt_reproject.h).  So on the buffer
 * prev_point_k = cur.eye_k + (d_k / |d|) * depth of step 3, formed in fp32 in that order, it returns trt_reproject's bits whenever the
 * cameras differ and z' is finite.  The tests of step 5 still compare the current normal with the history's: a surface that turned by more
 * than acos(normal_threshold) between the frames starts over.  Normals and lights are not interpolated.
 * Checks: trt_reproject's, in its order, with prev_point among the required buffers.  The history may be all NULL.  Host entry: 12 more
 * bytes per pixel are staged.  stats: as trt_reproject (the one kernel under TRT_K_DENOISE). */
int trt_reproject_motion(int device, const trt_reproject_params* params, int width, int height, const float* color, const float* variance,
                         const float* albedo, const float* normal, const float* depth, const float* prev_point, const float* prev_cv,
                         const float* prev_len, const float* prev_normal, const float* prev_depth, float* out_color, float* out_variance,
                         float* out_cv, float* out_len, trt_stats* stats);
/* The same with every buffer in DEVICE memory, as trt_reproject_device: nothing allocated, prev_cv and out_cv 16-byte aligned. */
int trt_reproject_motion_device(int device, const trt_reproject_params* params, int width, int height, const float* color, const float* variance,
                                const float* albedo, const float* normal, const float* depth, const float* prev_point, const float* prev_cv,
                                const float* prev_len, const float* prev_normal, const float* prev_depth, float* out_color, float* out_variance,
                                float* out_cv, float* out_len, void* hip_stream, trt_stats* stats);

/* trt_reproject for frames of ONE sample per pixel: the variance is not an input but estimated, from the history of the luminance's first
 * two moments where the history is long enough (the moments estimate of SVGF) and from the neighbourhood where it is not.  Inputs of the
 * current frame: color, albedo, normal, depth as for trt_reproject (no variance), and prev_point W*H*3 as for trt_reproject_motion or NULL.
 * History, all five or none: trt_reproject's four and
 *   prev_mom  W*H*4  (m1, m2, s, 0): the accumulated first and second moments of the demodulated luminance l = lum(c), and s = the sum of
 *                    the squared frame weights that make up the accumulated value (1 for one frame, 1 / N for a running mean of N, towards
 *                    alpha / (2 - alpha) under the exponential average); an earlier call's out_mom.
 * Outputs: trt_reproject's four and out_mom W*H*4.  Per pixel p = (x, y), stage A:
 *  1. Demodulate as trt_reproject's step 1 with variance := 0; l = lum(c).
 *  2. A pixel with no history (a miss, a NaN depth, a NULL history, a failed projection, W_s < 0.01) gives out_color = the input's bits,
 *     out_cv = (c, .), out_len = 1, out_mom = (l, l l, 1, 0).
 *  3. Otherwise (fx, fy, z') by trt_reproject's steps 3 and 4 if prev_point is NULL (the shortcut for byte-identical cameras included), by
 *     trt_reproject_motion's steps 3' and 4' from prev_point otherwise.
 *  4. Taps: trt_reproject's step 5 (order, tests, weights; per tap the depth is read, then the normal, cv, the length, mom); m1_h, m2_h, s_h
 *     = the weighted means of prev_mom over the counting taps, beside c_h and N_h.
 *  5. Blend: N and alpha' as trt_reproject's step 6, c' = c_h + alpha' (c - c_h); m1' = m1_h + alpha' (l - m1_h);
 *     m2' = m2_h + alpha' (l l - m2_h); s' = alpha'^2 + (1 - alpha')^2 s_h.  out_cv.rgb = c', out_len = N, out_color = c' a: the bits
 *     trt_reproject / trt_reproject_motion return on the same inputs (these do not depend on the variance).  out_mom = (m1', m2', s', 0).
 *  6. The TEMPORAL ROUTE: a hit pixel with N >= min_frames and 1 - s' >= 0.1.  There v = max(0, m2' - m1'^2) / (1 - s') and var' = v s':
 *     with frame weights a_i that sum to 1 over independent frames of variance sigma^2, E[m2 - m1^2] = sigma^2 (1 - sum a_i^2), and the
 *     accumulated colour has the variance sigma^2 sum a_i^2.
 * Stage B, a second kernel, for every hit pixel NOT on the temporal route (one predicate decides for both stages): the (2R+1)^2 window,
 * R = 3, rows outer, columns inner, over THIS frame's out_mom, normal and depth.  A tap q counts iff it is in the image and a hit; the centre
 * has w = 1, any other tap w = wn wz with trt_denoise's wn = max(0, n_p . n_q)^sigma_normal and
 * wz = exp(-|z_p - z_q| / (sigma_depth gz_p |q - p| + 1e-3 z_p)), gz_p trt_denoise's depth gradient, |q - p| by trt_sqrt.
 *     M1 = sum w m1_q / sum w,  M2 = sum w m2_q / sum w,  W2 = sum w^2 s_q / (sum w)^2;
 *     1 - W2 >= 0.1:  v = max(0, M2 - M1^2) / (1 - W2);
 *     otherwise the pixel stands alone behind its edges, nothing can be estimated, and v = M1^2: a relative standard deviation of 1, the
 *     conservative choice (the filter then smooths such a pixel as far as its edge-stopping weights let it);
 *     var' = v s'_p.
 * Both routes: out_cv.w = var', out_variance = var' max(lum(a), 1e-6)^2.  A miss: 0 and 0.
 * Arithmetic: fp32 in one fixed order, tinyraytracing_amd/csrc/trt_moments.h, which a CPU build of the same code reproduces bit for bit.
 * Non-finite or hostile values, prev_mom's included (a NaN, a negative s, s > 1), index nothing out of bounds; the results near them are
 * unspecified. */
typedef struct trt_moments_params {
    trt_reproject_params rp;
    int32_t min_frames;    /* the least history length of the temporal route, 1..255; 0 = 4 */
    int32_t sigma_normal;  /* stage B's normal exponent, 1..256; 0 = 128 */
    float sigma_depth;     /* stage B's depth sigma, >= 0; 0 = 1 */
} trt_moments_params;

/* On HOST buffers (staged for the call: 92 bytes per pixel, 12 more with prev_point, 52 more with a history).  TRT_EINVAL, in this order
 * before any device work: trt_reproject's checks in its order (required: the four inputs and the five outputs; the history: all five or
 * none), then min_frames outside 0..255, sigma_normal outside 0..256, a negative or NaN sigma_depth.  stats (optional): launches
 * [TRT_K_DENOISE] = 2 (stage A and stage B; stage B's blocks without a pixel for it return at once), kernel_ms[TRT_K_DENOISE], render_ms. */
int trt_reproject_moments(int device, const trt_moments_params* params, int width, int height, const float* color, const float* albedo,
                          const float* normal, const float* depth, const float* prev_point, const float* prev_cv, const float* prev_len,
                          const float* prev_normal, const float* prev_depth, const float* prev_mom, float* out_color, float* out_variance,
                          float* out_cv, float* out_len, float* out_mom, trt_stats* stats);
/* The same with every buffer in DEVICE memory, as trt_reproject_device: nothing allocated; prev_cv, out_cv, prev_mom and out_mom are read
 * and written as 16-byte records and must be 16-byte aligned (TRT_EINVAL otherwise).  TRT_MOMENTS_LDS=0 in the environment sends stage B
 * through its global-memory variant (an A/B switch; same bits). */
int trt_reproject_moments_device(int device, const trt_moments_params* params, int width, int height, const float* color, const float* albedo,
                                 const float* normal, const float* depth, const float* prev_point, const float* prev_cv, const float* prev_len,
                                 const float* prev_normal, const float* prev_depth, const float* prev_mom, float* out_color, float* out_variance,
                                 float* out_cv, float* out_len, float* out_mom, void* hip_stream, trt_stats* stats);

/* ---- firefly clamp: bound a pixel's luminance by its neighbourhood, before the history and the filter ------------------------------------
 * A stateless image-space operation shaped like trt_denoise: one W x H image, no scene handle, no state in the library.  It runs on the
 * frame's own buffers BEFORE trt_reproject* and trt_denoise: next-event estimation divides by the squared distance to the light sample, so
 * one sample close to a light is worth thousands of its neighbours, the filter spreads such a pixel into a blotch (its luminance weight is
 * relative to the pixel's own deviation), the history keeps it for 1 / alpha frames, and trt_reproject_moments' m2 carries it into every
 * pixel that later gathers it.  All buffers float, rows top to bottom:
 *   color W*H*3, albedo W*H*3 and depth W*H as for trt_denoise;
 *   variance W*H and out_variance W*H: both or neither (NULL);
 *   out_color W*H*3; out_scale W*H or NULL: the factor each pixel's colour was multiplied by.
 * No output may alias an input (a pixel reads its neighbours; not checked).  Per pixel p, window radius R, k = sigma:
 *  1. a = the demodulation factor and c = color / a as trt_denoise's step 1 (the same functions, variance 0), l_p = lum(c): the clamp works
 *     in the domain the filter and the history work in.
 *  2. A miss (depth >= TRT_INF, or a NaN) passes through: out_color and out_variance = the input's bits, out_scale = 1.
 *  3. The (2R+1)^2 window, rows outer and columns inner, the centre left out.  A tap q counts iff it is in the image, a hit, and l_q is
 *     finite.  n = the number of counting taps, S1 = sum l_q, S2 = sum l_q^2, accumulated in fp32 in that order.
 *  4. n < TRT_DS_MIN_TAPS: the pixel passes through (whatever its value: step 9).
 *  5. m = S1 / n,  v = max(0, S2 / n - m m),  T = m + k sqrt(v)   (trt_sqrt).
 *  6. l_p finite and l_p <= T: the pixel passes through.  A FLAT window, every counting tap equal to l_p, is this case with l_p = m = T; it is
 *     decided by comparing the taps, not by the rounded sums (the fp32 sum of n equal numbers over n may fall an ulp short of them), so that
 *     a constant image and the inside of a directly seen emitter keep their bits.
 *  7. l_p finite and l_p > T: s = T / l_p (one fp32 division), out_color = color s, out_variance = (variance s) s, out_scale = s.
 *  8. l_p or a colour channel not finite (and n >= TRT_DS_MIN_TAPS): the pixel is REPLACED, out_color = m a, out_variance = variance if that
 *     is finite, else 0, out_scale = 0.  This is the one place in the chain where a NaN sample can be stopped before it enters a history for good.
 *  9. With n < TRT_DS_MIN_TAPS such a pixel passes through, as in step 4.
 * What k = 3 leaves alone: with a fraction f of the window at luminance L and the rest near 0, m = f L and v = f (1 - f) L^2, so T >= L iff
 * f + k sqrt(f (1 - f)) >= 1; for k = 3 that is f >= 0.1.  A straight edge (5 of 8 taps at R = 1), the corner of a bright region (3 of 8) and
 * a bright line one pixel wide (2 of 8; 4 of 24 at R = 2) are therefore untouched whatever the contrast, and a lone bright pixel (0 of 8) is
 * brought down to T of its surroundings.  One bright tap among 8 is f = 0.125: of two ADJACENT fireflies neither is clamped at R = 1 (each
 * vouches for the other); at R = 2 (1 of 24) both are.
 * Limits: the clamp is BIASED, it removes energy (DESIGN.md has the measured amounts); it cannot tell an emitter or a highlight smaller than
 * a tenth of the window from a firefly and clamps both.  It is therefore OFF by default wherever the library offers it.
 * Arithmetic: fp32 in one fixed order, tinyraytracing_amd/csrc/trt_despeckle.h, which a CPU build of the same code reproduces bit for bit.
 * Hostile values (NaN, infinite or negative colours, albedos and depths) index nothing out of bounds. */
typedef struct trt_despeckle_params {
    int32_t radius;   /* window radius R, 1 or 2; 0 = 1 */
    float sigma;      /* k >= 0; 0 = 3 */
    uint32_t flags;   /* reserved, 0 */
} trt_despeckle_params;
#define TRT_DS_MIN_TAPS 3

/* On HOST buffers on `device` (HIP ordinal; a gfx950, else TRT_ENODEV), staged in device memory for the call (40 bytes per pixel, 4 more
 * each for variance, out_variance and out_scale).  params may be NULL (every default).  TRT_EINVAL, in this order before any device work:
 * a null required buffer (color, albedo, depth, out_color); variance without out_variance or the reverse; width or height < 1;
 * width * height > TRT_DENOISE_MAX_PIXELS; radius other than 0, 1 or 2; a negative or NaN sigma; nonzero flags.  stats (optional):
 * launches[TRT_K_DENOISE] = 1 (the one kernel), kernel_ms[TRT_K_DENOISE], render_ms = the call's device time (copies included); every other
 * field 0. */
int trt_despeckle(int device, const trt_despeckle_params* params, int width, int height, const float* color, const float* variance,
                  const float* albedo, const float* depth, float* out_color, float* out_variance, float* out_scale, trt_stats* stats);
/* The same with every buffer in DEVICE memory of `device`, the work enqueued on hip_stream (NULL = default stream); returns after that
 * stream has been synchronised.  Nothing but the stats crosses PCIe and no device memory is allocated.  TRT_DESPECKLE_LDS=0 in the
 * environment sends the taps to global memory instead of the block's LDS tile (an A/B switch; same bits). */
int trt_despeckle_device(int device, const trt_despeckle_params* params, int width, int height, const float* color, const float* variance,
                         const float* albedo, const float* depth, float* out_color, float* out_variance, float* out_scale, void* hip_stream,
                         trt_stats* stats);


/* ---- one node, several GPUs -------------------------------------------------------------------------------------
 * The sample/pixel loop has no cross-pixel dependency (main.cpp:84-108), so the image is tiled: the scene is replicated
 * on every device of the group, the rows of the tile are dealt to the devices in interleaved stripes of `row_block` rows
 * (device k renders the rows y with (y / row_block) % n == k), every device renders its stripes on its own host thread
 * (trt_render_device), and ONE ncclGather (RCCL over xGMI; /opt/rocm/include/rccl/rccl.h:745, communicators from
 * ncclCommInitAll :236) brings the packed stripes to devices[0], which un-interleaves them.  The random streams are keyed
 * by the global (pixel, sample), so the image is bit-identical to trt_render's for every n and every row_block.
 * RCCL is loaded (dlopen librccl.so.1) by trt_group_create only when the group spans more than one DISTINCT device;
 * a group whose entries name the same device several times (a rehearsal on a one-GPU box) gathers with device copies.
 * TRT_GROUP_FORCE_RCCL=1 in the environment at trt_group_create (a test switch) sends a group of ONE device through the
 * RCCL route as well — communicator of size 1, ncclGather to itself — so that the dlopen, the symbol bindings, the data type
 * constant and the stream ordering run on a one-GPU box.  Every device has a host thread of its own for the group's life. */
typedef struct trt_group trt_group;
int trt_group_create(const trt_scene* scene, int n_devices, const int* devices, trt_group** out);
/* p: as for trt_render (tile, spp, seed, flags); p->row_block (>= 1; 0 = 8) is the stripe height, row_mod / row_rem are
 * set by the library; the tile's first row p->y0 must be a multiple of row_block * group size (TRT_EINVAL otherwise: stripes are
 * counted from image row 0).  out_rgb_host: (y1-y0) * (x1-x0) * 3 floats.  stats (optional): rays / launches / kernel_ms summed
 * over the devices, render_ms = the slowest device's, plus gather_ms = gather + un-interleave on devices[0]. */
int trt_group_render(trt_group* g, const trt_params* p, float* out_rgb_host, trt_stats* stats, double* gather_ms);
/* The same with the image left in DEVICE memory of devices[0] (out_rgb_dev0: (y1-y0) * (x1-x0) * 3 floats there; nothing crosses
 * PCIe): what a caller that goes on working on the GPU links, and what bench.py --group times. */
int trt_group_render_device(trt_group* g, const trt_params* p, float* out_rgb_dev0, trt_stats* stats, double* gather_ms);
int trt_group_size(const trt_group* g);
void trt_group_destroy(trt_group* g);

const char* trt_last_error(void);

int trt_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* TRT_H */
