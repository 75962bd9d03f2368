/*
 * rtpbr.h — C ABI of the MI355X-native SDF path-tracing sample path.
 *
 * This is the drop-in boundary of SURVEY.md §8(b).  In the reference the boundary is the
 * Taichi kernel launch from Python: the kernels `pathtrace()` (src/pathtracer.py:94-103),
 * `refresh()` (src/renderer.py:12-22) and `post_process()` (src/postprocessor.py:24-43) take
 * no arguments and read/write global Taichi fields; the examples pass the camera by value
 * (examples/cornell_box/cornell_box_v3/renderer.py:11-42,
 *  examples/bunny/bunny_sdf_glass.py:393-432, examples/scene_demo/tokyo_ibl.py:403-439).
 * Here every field becomes a buffer owned by an opaque context and every kernel launch
 * becomes one plain C function, so that a ctypes / cgo / JNI / N-API stub can bind it.
 *
 * Conventions
 *   - every function returns 0 on success and a negative RTPBR_E* code on failure;
 *     rtpbr_last_error() returns a thread-local human readable message;
 *   - host pointers passed in are copied; the caller keeps ownership;
 *   - calls on one context are serialised on one HIP stream; different contexts
 *     (e.g. one per GPU) are independent; a context is not thread safe;
 *   - image buffers use the reference's field layout: dense (W, H, C) float32,
 *     element [i][j][c] with i = column from the left, j = row from the BOTTOM,
 *     j fastest.
 *
 * All structs are plain-old-data with 4-byte members only (no padding).
 */
#ifndef RTPBR_H
#define RTPBR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ error codes */
#define RTPBR_OK            0
#define RTPBR_EINVAL       -1   /* bad argument / inconsistent state            */
#define RTPBR_EHIP         -2   /* a HIP runtime call or kernel launch failed    */
#define RTPBR_ENOMEM       -3   /* allocation failed                             */
#define RTPBR_ESTATE       -4   /* call order violated (e.g. sample before scene)*/

/* ------------------------------------------------------------------ shapes
 * reference: class SHAPE(IntEnum) src/sdf.py:12-18.  RTPBR_SHAPE_BUNNY is the neural
 * SDF of examples/bunny/bunny_sdf_glass.py:149-203 (its own file calls it SHAPE_BUNNY=1). */
enum {
    RTPBR_SHAPE_NONE = 0,
    RTPBR_SHAPE_SPHERE = 1,
    RTPBR_SHAPE_BOX = 2,
    RTPBR_SHAPE_CYLINDER = 3,
    RTPBR_SHAPE_CONE = 4,
    RTPBR_SHAPE_PLANE = 5,
    RTPBR_SHAPE_BUNNY = 6
};

#define RTPBR_MAX_OBJECTS 32

/* ------------------------------------------------------------------ data model (T1..T5) */

/* reference: Ray src/dataclass.py:5-10 (40 B).  depth = raycast count, its SIGN is the
 * "finished" flag, 0 = fresh after refresh().  The examples' Ray has no depth. */
typedef struct rtpbr_ray {
    float   origin[3];
    float   direction[3];
    float   color[3];
    int32_t depth;
} rtpbr_ray;

/* reference: Material src/dataclass.py:13-20 (40 B).  emission is MULTIPLICATIVE,
 * (1,1,1) means "not a light". */
typedef struct rtpbr_material {
    float albedo[3];
    float emission[3];
    float roughness;
    float metallic;
    float transmission;
    float ior;
} rtpbr_material;

/* reference: Transform src/dataclass.py:23-28 (72 B).  rotation = Euler DEGREES,
 * scale = shape parameters (never a real scale), matrix = world->local rotation,
 * row major, filled by rtpbr_set_scene() like update_transform() src/scene.py:99-103. */
typedef struct rtpbr_transform {
    float position[3];
    float rotation[3];
    float scale[3];
    float matrix[9];
} rtpbr_transform;

/* reference: SDFObject src/dataclass.py:31-35 (116 B). */
typedef struct rtpbr_object {
    int32_t         type;
    rtpbr_transform transform;
    rtpbr_material  material;
} rtpbr_object;

/* reference: Camera src/dataclass.py:38-46 (52 B); vfov in degrees. */
typedef struct rtpbr_camera {
    float lookfrom[3];
    float lookat[3];
    float vup[3];
    float vfov;
    float aspect;
    float aperture;
    float focus;
} rtpbr_camera;

/* ------------------------------------------------------------------ variant knobs
 * One field per row of SURVEY.md Appendix B.  The reference fixes these as Python module
 * constants consumed through ti.static at JIT time (src/config.py:7-28 and the constant
 * block at the top of every example); here they are runtime values of one POD struct. */

enum { RTPBR_FORM_COMPLETE_PATH = 0,   /* examples: for i in range(MAX_RAYTRACE) inside the kernel */
       RTPBR_FORM_PERSISTENT_RAY = 1 };/* src/: one bounce-step per launch, state in ray_buffer   */

enum { RTPBR_MARCH_PLAIN = 0,          /* cornell_box.py:213-223, cornell_box_v2.py:186-196, shortest:63-72 */
       RTPBR_MARCH_RELAXED = 1,        /* cornell_box_v3/pathtracer.py:52-78 (err = d/t), tokyo, bunny      */
       RTPBR_MARCH_SRC = 2 };          /* src/scene.py:59-84 (origin moves, d < t*PIXEL_RADIUS)             */

enum { RTPBR_NORMAL_WORLD = 0,         /* examples: offsets in world space                   */
       RTPBR_NORMAL_LOCAL = 1 };       /* src/sdf.py:77-87: local frame, not rotated back    */

enum { RTPBR_RR_EXAMPLES = 0,          /* p = 1-exp(-i/light_quality); "kill" = color*=p, keep */
       RTPBR_RR_SRC = 1 };             /* p = (depth==0?1:q) - depth/MAX_RAYTRACE; kill = 0    */

enum { RTPBR_FRESNEL_C2 = 0,           /* F0=(e-1)/(e+1); F0*=2*F0  (cornell v1/v2/v3, bunny)  */
       RTPBR_FRESNEL_C4 = 1 };         /* F0=2(e-1)/(e+1); F0*=F0   (src, scene_demo, tokyo)   */

enum { RTPBR_HORIZON_KILL = 0,         /* examples: color *= (dot(D,n) > 0)                    */
       RTPBR_HORIZON_FLIP = 1 };       /* src/pbr.py:50-51: D = -D                             */

enum { RTPBR_ORIGIN_HIT = 0,           /* examples: origin = hit position                      */
       RTPBR_ORIGIN_OFFSET = 1 };      /* src/pbr.py:59-60: origin += +-n*MIN_DIS              */

enum { RTPBR_SURFACE_FULL = 0,
       RTPBR_SURFACE_DIFFUSE = 1 };    /* cornell_box_shortest.py:91-94                        */

enum { RTPBR_SKY_BLACK = 0,            /* cornell: miss => color = 0                           */
       RTPBR_SKY_ENVMAP = 1,           /* src/ibl.py:36-40, tokyo, bunny                       */
       RTPBR_SKY_GRADIENT = 2 };       /* scene_demo/main.py:245-248                           */

enum { RTPBR_PRIMARY_AS_SKY = 0,
       RTPBR_PRIMARY_BLACK = 1,        /* src BLACK_BACKGROUND, bunny_sdf.py:352               */
       RTPBR_PRIMARY_WHITE = 2 };      /* bunny_sdf_v2.py:355-356                              */

enum { RTPBR_TONEMAP_GAMMA_ACES_CLAMP = 0,  /* src, shortest, v3                               */
       RTPBR_TONEMAP_ACES_GAMMA = 1,        /* v1, v2                                          */
       RTPBR_TONEMAP_ACES_CLAMP_GAMMA = 2,  /* bunny*                                          */
       RTPBR_TONEMAP_ACES_GAMMA_CLAMP = 3 };/* tokyo, scene_demo                               */

enum { RTPBR_CAMERA_THIN_LENS = 0,     /* src/camera.py:11-36                                  */
       RTPBR_CAMERA_PINHOLE = 1 };     /* cornell_box_shortest.py:107-118 (no lens draws)      */

typedef struct rtpbr_config {
    int32_t  width, height;        /* image_resolution                                        */
    uint32_t seed;                 /* counter-based RNG seed                                  */
    int32_t  kernel_form;          /* RTPBR_FORM_*                                            */
    int32_t  max_raymarch;         /* MAX_RAYMARCH                                            */
    int32_t  max_raytrace;         /* MAX_RAYTRACE                                            */
    /* sphere tracing */
    int32_t  march_kind;           /* RTPBR_MARCH_*                                           */
    float    min_dis;              /* examples: march start t0; src: normal offset MIN_DIS    */
    float    max_dis;              /* MAX_DIS                                                 */
    float    hit_eps;              /* PRECISION (plain) or PIXEL_RADIUS (relaxed / src)       */
    float    omega0;               /* initial over-relaxation                                 */
    int32_t  omega_guard;          /* 1: fall back only while omega > 1                       */
    float    omega_fb_a, omega_fb_b; /* on overshoot: omega <- a + b*omega                    */
    /* sdf */
    float    box_round;            /* rounding rho of sd_box                                  */
    int32_t  nearest_init;         /* 0: start from object 0 (cornell_box_v3/pathtracer.py:41-49)
                                      1: start from (0, MAX_DIS) (src/scene.py:45-46, tokyo_ibl.py:222) */
    /* normal */
    float    normal_h;
    int32_t  normal_space;         /* RTPBR_NORMAL_*                                          */
    /* russian roulette */
    int32_t  rr_kind;              /* RTPBR_RR_*                                              */
    float    light_quality;        /* examples                                                */
    float    quality_per_sample;   /* src QUALITY_PER_SAMPLE                                  */
    /* surface model */
    int32_t  surface_kind;         /* RTPBR_SURFACE_*                                         */
    int32_t  fresnel_kind;         /* RTPBR_FRESNEL_*                                         */
    int32_t  fresnel_roughness_mix;/* examples 1, src 0                                       */
    int32_t  below_horizon;        /* RTPBR_HORIZON_*                                         */
    int32_t  origin_mode;          /* RTPBR_ORIGIN_*                                          */
    float    env_ior;              /* ENV_IOR                                                 */
    /* miss / sky */
    int32_t  sky_kind;             /* RTPBR_SKY_*                                             */
    int32_t  primary_miss;         /* RTPBR_PRIMARY_*                                         */
    /* stop test: stop if brighter, or visible < vis_lo, or visible > vis_hi */
    float    vis_lo, vis_hi;
    /* camera */
    int32_t  camera_kind;          /* RTPBR_CAMERA_*                                          */
    /* tone map */
    int32_t  tonemap_order;        /* RTPBR_TONEMAP_*                                         */
    int32_t  aces_truncated;       /* 1: cornell_box_shortest.py:126-128 literals             */
    float    exposure;
    float    gamma;
    /* animation uniform (u_frame, bunny_sdf_glass.py:213-217) */
    int32_t  frame;
    /* persistent-ray form: bounce-steps per pixel per launch (SAMPLES_PER_PIXEL) */
    int32_t  steps_per_launch;
    /* self-adaptive sampling (src/config.py:14,17; persistent-ray form only): a pixel is sampled
     * only while its running mean display-space change diff_pixels exceeds noise_threshold */
    int32_t  adaptive_sampling;
    float    noise_threshold;
    /* neural-bunny animation: amplitude of the vertical bob p.z += anim_bob * sin(t) after the frame rotation
     * (bunny_sdf_glass.py:216 and bunny_sdf_v2.py:216: 0.1; bunny_sdf.py:213-214 rotates only: 0) */
    float    anim_bob;
} rtpbr_config;

/* ------------------------------------------------------------------ buffers */
enum { RTPBR_BUF_IMAGE_BUFFER = 0,   /* T7 image_buffer  (W,H,4) f32: (sum r, sum g, sum b, count) */
       RTPBR_BUF_IMAGE_PIXELS = 1,   /* T8 image_pixels  (W,H,3) f32 display colour                */
       RTPBR_BUF_RAY_BUFFER   = 2,   /* T6 ray_buffer    (W,H) of rtpbr_ray (persistent-ray form)  */
       RTPBR_BUF_DIFF_BUFFER  = 3,   /* T11 diff_buffer  (W,H,2) f32 (sum of display change, count) src/fileds.py:21 */
       RTPBR_BUF_DIFF_PIXELS  = 4,   /* T11 diff_pixels  (W,H) f32                                  src/fileds.py:22 */
       /* first-hit features (rtpbr_render_features) and the denoised image (rtpbr_denoise): allocated on first use,
        * RTPBR_ESTATE before; outputs only (rtpbr_write_buffer: RTPBR_EINVAL) */
       RTPBR_BUF_FEAT_ALBEDO  = 5,   /* (W,H,3) f32 material.albedo of the first hit, 0 on a miss                   */
       RTPBR_BUF_FEAT_NORMAL  = 6,   /* (W,H,3) f32 shading normal as the sample path computes it (calc_normal with
                                      *           cfg.normal_space: local-frame normals stay local), 0 on a miss     */
       RTPBR_BUF_FEAT_DEPTH   = 7,   /* (W,H)   f32 length(hit - ray origin), cfg.max_dis on a miss                 */
       RTPBR_BUF_FEAT_OBJECT  = 8,   /* (W,H)   i32 index of the hit object in the set_scene array, -1 on a miss    */
       RTPBR_BUF_DENOISED_PIXELS = 9, /* (W,H,3) f32 denoised display colour                                       */
       /* written by rtpbr_reproject / rtpbr_reproject_scene: allocated on the first such call, RTPBR_ESTATE before; output only */
       RTPBR_BUF_MOTION       = 10,  /* (W,H,2) f32 old-frame pixel coordinates each pixel drew its history from,
                                      *           (-1,-1) = no history (rtpbr_reproject)                           */
       /* noise estimation (rtpbr_noise_update / rtpbr_noise_estimate): allocated on first use, RTPBR_ESTATE before;
        * outputs only */
       RTPBR_BUF_MOMENTS      = 11,  /* (W,H,4) f32 moments of the batch means' linear luminance: (sum c L, sum c L^2, sum c, K) */
       RTPBR_BUF_NOISE        = 12,  /* (W,H)   f32 estimated standard deviation of lum(r(displayed average))          */
       /* the pixel selection (rtpbr_select_mask / rtpbr_select_noisy): allocated on the first select call, RTPBR_ESTATE before;
        * output only */
       RTPBR_BUF_SELECTION    = 13,  /* (W,H)   u8  1 = selected: what rtpbr_sample_selected traces (select_tiers > 1: 1 + tier) */
       /* the packed 8-bit frame (rtpbr_present): allocated on the first present, RTPBR_ESTATE before; output only.  NOT in the
        * field layout: (H,W,C) u8, row 0 = the TOP row of the picture, x fastest, C = 3 or 4 as the last present said */
       RTPBR_BUF_PRESENT      = 14,
       /* the two halves and the error estimate of the denoised frame (rtpbr_half_update / rtpbr_denoise_error): each allocated on
        * the first such call, RTPBR_ESTATE before; outputs only */
       RTPBR_BUF_HALF_BUFFER  = 15,  /* (W,H,4) f32 half A's (sum r, sum g, sum b, count); half B = image_buffer - A per component */
       RTPBR_BUF_DENOISED_ERROR = 16, /* (W,H) f32 estimated standard deviation of lum(rtpbr_denoise's display colour)         */
       /* the weight of rtpbr_denoise_blend: allocated by its first call, freed by rtpbr_set_config with a new resolution; output only */
       RTPBR_BUF_BLEND_WEIGHT = 17,  /* (W,H) f32 t in [0, 1]: 1 = the denoised colour, 0 = the raw average (rtpbr_denoise_blend_levels: T_K) */
       /* the depth of rtpbr_denoise_blend_levels: allocated by its first call (which allocates the weight too), freed by
        * rtpbr_set_config with a new resolution; output only */
       RTPBR_BUF_BLEND_DEPTH  = 18,  /* (W,H) f32 in 0..K: K = the whole filter was kept, 0 = the raw average                   */
       /* the error estimate of the level-blended frame (rtpbr_blend_error): allocated by its first call, freed by rtpbr_set_config
        * with a new resolution; output only */
       RTPBR_BUF_BLEND_ERROR  = 19 };   /* (W,H) f32 estimated root-mean-square error of lum(rtpbr_denoise_blend_levels' display
                                         *           colour): variance and the bias the halves can see                         */

enum { RTPBR_ENV_RGB8 = 0,           /* uint8 (W_e,H_e,3), [x][y], y=0 bottom: what ti.tools.imread gives */
       RTPBR_ENV_RGB32F = 1 };       /* float32 (W_e,H_e,3) already preprocessed (T9 as is)               */

/* Work counters of the last rtpbr_sample() call (B-bar, S-bar). */
typedef struct rtpbr_counters {
    uint64_t samples;       /* pixel-samples (complete-path) or bounce-steps (persistent) */
    uint64_t raycasts;      /* raycast() calls                                            */
    uint64_t march_steps;   /* nearest() evaluations inside raycast loops                 */
    uint64_t hits;          /* surface interactions                                       */
    uint64_t sky_lookups;   /* environment lookups                                        */
    uint64_t deposits;      /* image_buffer accumulations                                 */
} rtpbr_counters;

typedef struct rtpbr_ctx rtpbr_ctx;

/* ------------------------------------------------------------------ entry points */

/* Create a context on HIP device `device`.  Replaces ti.init(arch=...) (src/config.py:5)
 * plus field allocation (src/fileds.py:7-15). */
int rtpbr_create(int device, rtpbr_ctx** out);
int rtpbr_destroy(rtpbr_ctx* ctx);
const char* rtpbr_last_error(void);
/* Name of the backend ("hip-gfx950"); lets callers assert which library they loaded. */
const char* rtpbr_backend(void);

/* Replaces the module constants of src/config.py:7-28.  (Re)allocates the per-pixel
 * buffers zero-initialised when the resolution changes. */
int rtpbr_set_config(rtpbr_ctx* ctx, const rtpbr_config* cfg);

/* Replaces the element-wise copy into the `objects` field (src/scene.py:38-41) and
 * build_scene()/update_all_transform() (src/scene.py:106-113): the world->local
 * matrices are computed here from `rotation`.  `scale10` != 0 multiplies position and
 * scale by 10 (cornell_box_v3/sdf.py:16-18). */
int rtpbr_set_scene(rtpbr_ctx* ctx, const rtpbr_object* objects, int n, int scale10);
/* Read back the uploaded table (with matrices filled), n entries. */
int rtpbr_get_scene(rtpbr_ctx* ctx, rtpbr_object* objects, int n);

/* Replaces the 0-d camera fields (src/camera.py:119-129) / the camera kernel arguments
 * (cornell_box_v3/renderer.py:12-16). */
int rtpbr_set_camera(rtpbr_ctx* ctx, const rtpbr_camera* cam);

/* Replaces Image(path) + Image.process(exposure, gamma) (src/ibl.py:14-23,32-33).
 * RGB8 texels are converted as (c/255*exposure)^gamma; RGB32F texels are used as is. */
int rtpbr_set_env(rtpbr_ctx* ctx, const void* texels, int w, int h, int fmt,
                  float exposure, float gamma);

/* Per-shape data blobs.  Only RTPBR_SHAPE_BUNNY takes one: the 625 weights of the neural
 * SDF (examples/bunny/bunny_sdf_glass.py:157-201, inline literals in the reference). */
int rtpbr_set_shape_data(rtpbr_ctx* ctx, int shape, const float* data, int n);

/* Tile partition of the frame for multi-GPU rendering: tiles of
 * tile_w x tile_h pixels are dealt round-robin, tile t belongs to rank t % world.
 * (0,0,0,1) or world==1 means "the whole frame". */
int rtpbr_set_tiles(rtpbr_ctx* ctx, int tile_w, int tile_h, int rank, int world);

/* refresh() src/renderer.py:12-22: zero image_buffer, ray_buffer.depth = 0. */
int rtpbr_refresh(rtpbr_ctx* ctx);

/* The hot path.  complete-path form: `n` samples per owned pixel are traced and
 * accumulated (the spp loop of cornell_box_v3/renderer.py:31-36).  persistent-ray form:
 * `n` launches of pathtrace() (src/renderer.py:29-30), each advancing every pixel by
 * cfg.steps_per_launch bounce-steps.  Asynchronous: returns after enqueue. */
int rtpbr_sample(rtpbr_ctx* ctx, int n);

/* post_process() src/postprocessor.py:24-43: image_buffer -> image_pixels. */
int rtpbr_post_process(rtpbr_ctx* ctx);

/* ---- First-hit features and an edge-aware a-trous denoise (Dammertz et al. 2010), the filter the reference's
 * post_process() leaves open (src/postprocessor.py:30 "# ToDo: Post Denoise").
 *
 * rtpbr_render_features: one primary ray through each pixel CENTRE (the camera ray with both jitters 0.5 and no lens
 *   offset: origin = lookfrom for thin lens and pinhole alike; no RNG draws), marched with cfg.march_kind over the current
 *   scene, camera, configuration, shape data and frame uniform; fills RTPBR_BUF_FEAT_*.  Does not touch the work counters.
 * rtpbr_denoise: writes RTPBR_BUF_DENOISED_PIXELS only, from image_buffer as rtpbr_post_process reads it; renders the
 *   features first when they are missing or stale (after rtpbr_set_config / set_scene / set_camera / set_shape_data).
 *   p == NULL: the defaults below.  The filter, per pixel p with count a_p > 0:
 *     c = (b.x/b.w, b.y/b.w, b.z/b.w), divided per channel by max(albedo_p, 1e-3f) if demodulate;
 *     level k = 0 .. iterations-1, step s = 2^k: dy = -2..2 (outer), dx = -2..2 (inner), q = p + s (dx, dy), q skipped when
 *       outside the frame, without samples or on another object index (hit and miss never mix);
 *       h = H[|dx|] H[|dy|], H = {3/8, 1/4, 1/16};  r(c) = c / (1 + c) per channel;  |v|^2 = (x*x + y*y) + z*z;
 *       e = ((|r(c_p) - r(c_q)|^2 ic_k + |n_p - n_q|^2 in) + ((z_p - z_q) / max(z_p, 1e-6f))^2 iz) + |a_p - a_q|^2 ia;
 *       w = h exp(-min(e, 80)) (the Cephes exp of the sample path);  c_p <- sum w c_q / sum w, accumulated in tap order;
 *     ic_0 = 1 / (sigma_color * sigma_color) in f32, ic_k = ic_0 4^k (sigma_color halves per level); in, iz, ia alike;
 *     remodulate (x max(albedo_p, 1e-3f)) if demodulate; denoised = the configured tone map of (c, 1).
 *   Pixels with count 0 show exactly what rtpbr_post_process shows and are nobody's neighbour.  iterations = 0 with
 *   demodulate = 0 reproduces image_pixels bit for bit.
 *   The albedo is a per-object constant (0 on a miss) and taps never cross object indices, so a_q = a_p on every tap taken:
 *   the albedo term is always 0 and sigma_albedo has NO effect on the result (it is validated like the others and kept for
 *   the ABI; do not tune it).  The kernels skip the term; the definition above is what they compute.
 * Option "denoise_fill" (rtpbr_set_option; 0 or 1, default 0): with 0 everything above holds, bit for bit.  With 1, rtpbr_denoise —
 *   and only it: rtpbr_denoise_guided, rtpbr_denoise_coverage, rtpbr_denoise_error, the blend family, rtpbr_post_process and
 *   rtpbr_present ignore the option and keep their bytes — reconstructs the pixels without samples from their neighbours.  Such
 *   pixels are what rtpbr_reproject / rtpbr_reproject_scene leave where the new view sees what the old one did not, and what
 *   rtpbr_select_mask + rtpbr_sample_selected leave unselected (a lattice of one pixel in four, say).
 *     A pixel is LIVE at level k when it has a colour on entry to that level: at level 0 the pixels with image_buffer[p].w > 0;
 *     the rest are EMPTY.  Tap set, tap order, h, the sums (from +0, no fma), ic_k / in / iz, the clamp min(e, 80) and the exp
 *     are the filter's above.  A tap q is skipped, for live and empty centres alike, when it is outside the frame, when it is
 *     not live on entry to this level, or when RTPBR_BUF_FEAT_OBJECT[q] != RTPBR_BUF_FEAT_OBJECT[p].
 *     Live centre: the level above, operation for operation; the only difference is who is live — a pixel filled at an earlier
 *       level is a tap like any other.
 *     Empty centre p (its features are valid: they are rendered for every pixel): the same loop with the colour term of e taken
 *       as +0, e = |n_p - n_q|^2 in + ((z_p - z_q) / max(z_p, 1e-6f))^2 iz (left to right), w = h exp(-min(e, 80)).  If
 *       sum w > 0 after the loop, c_p = sum w c_q / sum w: p is live from the next level on and counts as FILLED AT LEVEL k.
 *       Otherwise p stays empty.  Every level reads only its input: a fill never sees another fill of the same level.
 *     Demodulation: at level 0 a tap's colour is its average divided by max(albedo_p, 1e-3f) — the centre's own albedo, which is
 *       the tap's (one constant per object); a filled pixel is remodulated by its own albedo at the last level.
 *     Last level: a pixel live on entry or filled there shows the configured tone map of its remodulated (c, 1); a pixel still
 *       empty shows what rtpbr_post_process shows.
 *     h >= 1/256 and exp(-80) ~ 1.8e-35, their product is a normal float: an empty pixel is filled at level k exactly when some
 *       tap of that level is live on its object — a rule about reach (2 * 2^k pixels per axis), not about weights.
 *   So: with iterations = 1 every pixel that has samples carries the bytes it has with the option off; on a frame where every
 *   pixel has samples both settings give the same bytes at every iterations; iterations = 0 is the same call either way and
 *   fills nothing.  image_buffer, the features, the selection, the noise moments, the halves, the work counters and sample_base
 *   are untouched, and the refusals are those below.  rtpbr_get_counter names "fill_filled" (pixels that were empty at level 0
 *   and got a colour), "fill_empty" (pixels still empty at the end) and "fill_deepest" (the highest level at which a pixel was
 *   filled, 0 when none was) describe the last rtpbr_denoise that ran with the option at 1 and iterations > 0 (0 before any such
 *   call; a refused call leaves them); they are counted by the filter's kernels, and reading them blocks.
 * Both return RTPBR_ESTATE with tiles of world > 1 (whole frames only) and RTPBR_EINVAL for bad parameters
 * (iterations outside 0..8, demodulate not 0/1, a sigma that is not finite and > 0 or whose 1/sigma^2 overflows, a
 * sigma_color whose 1/sigma^2 * 4^(iterations-1) overflows). */
typedef struct rtpbr_denoise_params {   /* 4-byte members, no padding */
    int32_t iterations;    /* a-trous levels 0..8, step 2^k; 0 = tone map only                  */
    int32_t demodulate;    /* 1: filter radiance / max(albedo, 1e-3), multiply back             */
    float   sigma_color, sigma_normal, sigma_depth, sigma_albedo;   /* all > 0; sigma_albedo has no effect (see above) */
} rtpbr_denoise_params;
/* Defaults (p == NULL), measured on Cornell v3 (256x256, 4 spp) and the src/ Tokyo scene (256x144, 16 bounce-steps) against
 * converged frames: the best worst case of 120 settings, display RMSE 0.235x / 0.279x the noisy frame's (DESIGN.md section 6b,
 * examples/denoise_sweep.py).  raytracingpbr_amd.dataclass.DenoiseParams.DEFAULTS mirrors them (tests/test_feature_ref.py checks). */
#define RTPBR_DENOISE_DEFAULT_ITERATIONS   4
#define RTPBR_DENOISE_DEFAULT_DEMODULATE   0
#define RTPBR_DENOISE_DEFAULT_SIGMA_COLOR  2.0f
#define RTPBR_DENOISE_DEFAULT_SIGMA_NORMAL 0.3f
#define RTPBR_DENOISE_DEFAULT_SIGMA_DEPTH  0.2f
#define RTPBR_DENOISE_DEFAULT_SIGMA_ALBEDO 0.1f
int rtpbr_render_features(rtpbr_ctx* ctx);
int rtpbr_denoise(rtpbr_ctx* ctx, const rtpbr_denoise_params* p);

/* ---- Temporal reuse: keep the accumulated samples across a camera move by reprojecting them into the new view.
 *
 * rtpbr_reproject(ctx, new_cam, p) replaces rtpbr_set_camera(new_cam) + rtpbr_refresh() for a host that wants to keep
 * history (the reference clears on every moving frame: src/renderer.py:25-32).  In order:
 *   1. flushes lazy shading and orders itself behind asynchronous read-backs of image_buffer, ray_buffer and the diff
 *      buffers (as rtpbr_refresh does; an outstanding rtpbr_read_buffer_async of image_buffer lands the pre-call contents);
 *   2. renders the features of the current (old) camera if they are stale;
 *   3-4. keeps the old camera frame, and copies image_buffer, the (normal, depth) records and the object indices into
 *      internal history buffers (copies: every address rtpbr_buffer_device_ptr handed out stays valid);
 *   5. applies new_cam exactly as rtpbr_set_camera does;
 *   6. renders the features of the new camera into RTPBR_BUF_FEAT_* (a following rtpbr_denoise does not render them again);
 *   7. gathers the history into image_buffer and writes RTPBR_BUF_MOTION (below);
 *   8. resets what rtpbr_refresh resets except image_buffer: ray_buffer.depth = 0 (in-flight persistent-form paths belong
 *      to the old camera) and, with adaptive sampling, diff_buffer = (1,1), diff_pixels = 1e32.
 * sample_base is not reset (neither does rtpbr_refresh): samples taken afterwards continue the RNG sequence and never repeat
 * the history's.  The work counters are untouched.
 *
 * The gather, per new pixel p = (x, y) with new features (z_new, n_new, obj_new) — every operation in f32, in this order,
 * fused only where fma3(s, b, a) = (fmaf(s, b.x, a.x), ...) is written; dot(a, b) = fmaf(a.z, b.z, fmaf(a.y, b.y, a.x*b.x)),
 * length(a) = sqrtf(dot(a, a)), normalize(a) = a * (1 / sqrtf(dot(a, a))), cross as usual (no fma):
 *   d = normalize(fma3(v, ver1, fma3(u, hor1, llc1)) - lf1), u, v as rtpbr_render_features computes them;
 *   hit (obj_new >= 0): D = fma3(z_new, d, lf1) - lf0 (the first hit seen from the old eye);
 *   miss (obj_new = -1): D = d (a point at infinity: every sky kind depends on the direction only);
 *   N = cross(hor0, ver0);  s = dot(llc0 - lf0, N) / dot(D, N);  no history unless s > 0 (behind the old camera, or NaN);
 *   P = D * s - (llc0 - lf0);  u0 = dot(P, hor0) / dot(hor0, hor0);  v0 = dot(P, ver0) / dot(ver0, ver0);
 *   px = u0 * W - 0.5f, py = v0 * H - 0.5f;  no history unless -1 < px < W and -1 < py < H;
 *   per axis: x0 = floorf(px), fx = px - x0; fx < 2^-10: fx = 0; fx > 1 - 2^-10: x0 = x0 + 1, fx = 0 (the snap: an
 *     unchanged camera reproduces the buffer exactly); the same for y;
 *   taps (0,0), (1,0), (0,1), (1,1) in this order at (x0 + i, y0 + j), weight ((1 - fx) or fx) * ((1 - fy) or fy); a tap of
 *     weight 0 is skipped; a tap is accepted if it lies inside the frame, its old count is > 0, its old object equals
 *     obj_new and, on a hit, |z_old - L| <= depth_tolerance * L with L = length(D), and (normal_cos <= -1 or
 *     dot(n_old, n_new) >= normal_cos);
 *   S = S + w * b_q, Wt = Wt + w over accepted taps (from 0, in tap order, per component); b = S / Wt per component;
 *   if b.w > max_history: b = b * (max_history / b.w) (all four components, one quotient);
 *   no accepted tap: b = 0, motion = (-1, -1); otherwise motion = (x0 + fx, y0 + fy) after the snap.
 * lf/llc/hor/ver: the camera frames of rtpbr_set_camera (0 = old, 1 = new).  Counts become fractional; rtpbr_post_process and
 * rtpbr_denoise divide by the count as before.
 *
 * Known bias.  History is reused as if radiance did not depend on the view: on glossy and refractive surfaces the history
 * shows the old view's reflections until new samples outweigh it.  A thin-lens camera's history was rendered with defocus
 * but is reprojected through the lens centre.  max_history bounds both: the history never weighs more than max_history
 * samples.  Objects that moved rigidly: rtpbr_reproject_scene below.  An animated frame, changes of shape or material and
 * tiles of world > 1 are out of scope (see the errors).
 *
 * Errors: RTPBR_EINVAL for a NULL context or camera and for bad parameters (max_history not finite and > 0,
 * depth_tolerance not finite and >= 0, normal_cos not within -1..1); RTPBR_ESTATE before set_config / set_scene /
 * set_camera, with tiles of world > 1, for the bunny without its shape data, and when rtpbr_set_config, set_scene,
 * set_shape_data or set_env ran since the last rtpbr_refresh or rtpbr_reproject: history from another scene,
 * configuration, animation frame or environment is not history.  A refused call changes nothing. */
typedef struct rtpbr_reproject_params {   /* 4-byte members, no padding */
    float max_history;       /* cap on a pixel's count after the warp (> 0, finite)                 */
    float depth_tolerance;   /* relative: |z_old - |X - lookfrom_old|| <= tol * |X - lookfrom_old|  */
    float normal_cos;        /* a tap needs dot(n_old, n_new) >= normal_cos (-1 disables the test)  */
} rtpbr_reproject_params;
/* Defaults (p == NULL), measured over an 11-move pan plus dolly on Cornell v3 (256x256, 4 spp per frame) and the src/ Tokyo
 * scene (256x144, 4 bounce-steps per frame) against converged frames: the best of 45 settings, display RMSE 0.516x / 0.324x
 * that of refreshing on every move (examples/reproject_flythrough.py --sweep).  On these scenes the
 * object test does most of the work: with the normal test off (-1) and a loose depth tolerance the score is 0.8 % better than
 * with (64, 0.05, 0.9).  raytracingpbr_amd.dataclass.ReprojectParams.DEFAULTS mirrors them (tests/test_reproject_ref.py checks). */
#define RTPBR_REPROJECT_DEFAULT_MAX_HISTORY     64.0f
#define RTPBR_REPROJECT_DEFAULT_DEPTH_TOLERANCE 0.2f
#define RTPBR_REPROJECT_DEFAULT_NORMAL_COS      -1.0f
int rtpbr_reproject(rtpbr_ctx* ctx, const rtpbr_camera* new_cam, const rtpbr_reproject_params* p);

/* ---- Temporal reuse across rigid object motion.
 *
 * rtpbr_reproject_scene(ctx, new_cam, new_objects, n, scale10, p) replaces rtpbr_set_scene(new_objects, n, scale10) + an
 * optional rtpbr_set_camera(new_cam) + rtpbr_refresh() for a host whose objects moved rigidly (translated and / or rotated) and
 * that wants to keep history.  new_cam == NULL: the camera stays.  p == NULL: rtpbr_reproject's defaults.
 *
 * Only rigid motion is accepted.  The check is made on the table as rtpbr_set_scene would store it (after scale10 has
 * multiplied position and scale by ten): n must equal the current object count, and for every i the type, the three scale
 * words and the ten material words must equal the current table's bit for bit.  Anything else: RTPBR_EINVAL, "not a rigid
 * motion: use rtpbr_set_scene + rtpbr_refresh".
 * Object k is MOVED when any of its 3 position words or 9 matrix words differs bitwise between the old and the new stored
 * table (the matrix as rtpbr_set_scene computes it from `rotation`: a turn of 360 degrees that yields the same matrix is no
 * move, whatever the rotation words say).
 *
 * In order — steps 1-4 and 6-8 are those of rtpbr_reproject:
 *   1. flushes lazy shading and orders itself behind asynchronous read-backs, as rtpbr_reproject does;
 *   2. renders the features of the current (old) scene and camera if they are stale;
 *   3-4. keeps the old camera frame and the old stored position and matrix of every object, and copies image_buffer, the
 *      (normal, depth) records and the object indices into the internal history buffers;
 *   5. applies new_objects exactly as rtpbr_set_scene does (matrices, rotation signature, scene kind, upload; the host waits
 *      for the stream there, as in rtpbr_set_scene), then new_cam exactly as rtpbr_set_camera does if it is not NULL;
 *   6. renders the features of the new scene and camera into RTPBR_BUF_FEAT_*;
 *   7. gathers the history into image_buffer and writes RTPBR_BUF_MOTION (below);
 *   8. resets what rtpbr_reproject resets: ray_buffer.depth = 0 and, with adaptive sampling, the diff buffers; with moments
 *      (rtpbr_noise_update) they are warped with the image and the snapshot becomes the warped image_buffer.
 * The call ends with valid history and valid features; sample_base and the work counters are untouched.
 *
 * The gather is rtpbr_reproject's, operation for operation (dot, fma3, length, the projection, the snap, the four taps, the
 * acceptance tests, the weights, the max_history cap, the moments rule), except for D and the normal compared on a hit
 * (obj_new = k >= 0) on a MOVED object.  R = the row-major world-to-local matrix, p = the position, 0 = old, 1 = new:
 *   X1 = fma3(z_new, d, lf1);  a = X1 - p1 (per component);
 *   l = (dot(R1 row 0, a), dot(R1 row 1, a), dot(R1 row 2, a))                      (the hit in the object's frame)
 *   X0.c = dot((R0[0][c], R0[1][c], R0[2][c]), l) + p0.c  for c = x, y, z           (where that point was in the old world)
 *   D = X0 - lf0;  L = length(D) enters the depth test as before;
 *   the normal of the normal_cos test: with cfg.normal_space == RTPBR_NORMAL_WORLD, m = (dot(R1 row r, n_new)) for r = 0..2,
 *     n' = (dot(R0 column c, m)) for c = 0..2, and the test is dot(n_old, n') >= normal_cos; with RTPBR_NORMAL_LOCAL the
 *     stored normals are in the object's frame already and n_new is compared as it is.
 * A hit on an object that did not move: D = fma3(z_new, d, lf1) - lf0 and n_new; a miss: D = d — rtpbr_reproject's
 * expressions, so with no moved object the call writes exactly what rtpbr_reproject(new_cam) writes (image_buffer,
 * RTPBR_BUF_MOTION, the moments, the snapshot).  RTPBR_BUF_MOTION now carries object motion too: a pixel on a moved object
 * under a still camera reports where that surface point was in the old frame.
 *
 * Known bias, beyond rtpbr_reproject's.  The history of EVERY pixel, on a moved object or not, was lit by the old scene: it
 * carries the old frame's shadows and interreflections of the moved objects (the shadow a box left behind fades, the one
 * where it went builds up), and a moved object's own history carries the light of where it was.  No test detects this;
 * max_history is the only bound, so use a smaller value than for camera moves (DESIGN.md section 6h has the measured
 * numbers, examples/reproject_moving.py --sweep reproduces them).
 *
 * Errors, every one before anything changes: all RTPBR_EINVAL and RTPBR_ESTATE cases of rtpbr_reproject (a NULL new_cam is
 * valid here), RTPBR_EINVAL also for NULL new_objects and for a table that fails the rigidity check; RTPBR_ESTATE when the
 * history is not valid — this call does not repair history an earlier rtpbr_set_scene (or set_config, a changed cfg.frame
 * included, set_shape_data, set_env) broke — and with tiles of world > 1.  Changes of shape, scale or material and the
 * bunny's animation frame stay out of scope: rtpbr_set_scene / rtpbr_set_config + rtpbr_refresh. */
int rtpbr_reproject_scene(rtpbr_ctx* ctx, const rtpbr_camera* new_cam, const rtpbr_object* new_objects, int n, int scale10,
                          const rtpbr_reproject_params* p);

/* ---- Per-pixel noise estimation and a variance-guided a-trous (the spatial half of SVGF, Schied et al. 2017).
 *
 * Notation: r(c) = c / (1 + c) per channel (as rtpbr_denoise); lum(c) = (0.299f * c.x + 0.587f * c.y) + 0.114f * c.z.  Every
 * operation is f32, in the order written, nothing fused.
 *
 * rtpbr_noise_update folds the samples deposited into image_buffer since the last update into RTPBR_BUF_MOMENTS, using an
 *   internal snapshot s of image_buffer (both allocated zeroed on the first call: everything accumulated until then is the
 *   first batch).  Per pixel, b = image_buffer:
 *     d = b - s per component; cnt = d.w;
 *     if cnt > 0: m = (d.x / cnt, d.y / cnt, d.z / cnt); L = lum(m) (linear: see below); cL = cnt * L;
 *                 M.x = M.x + cL; M.y = M.y + cL * L; M.z = M.z + cnt; M.w = M.w + 1;
 *     s = b (in every case).
 *   So M = (sum c L, sum c L^2, sum c, K) over K batches of c_k samples.  It flushes lazy shading, is ordered behind
 *   asynchronous reads of the moments, and writes nothing else.
 *   rtpbr_refresh zeroes M and s when they exist; rtpbr_set_config with a new resolution frees them and RTPBR_BUF_NOISE;
 *   rtpbr_write_buffer(RTPBR_BUF_IMAGE_BUFFER) re-takes s (written data is no batch); rtpbr_reproject warps M (below).
 *
 * rtpbr_noise_estimate writes RTPBR_BUF_NOISE = sqrt(v) (correctly rounded) per pixel and, if out != NULL, the statistics;
 *   it blocks like rtpbr_get_counters.  It renders the features first when they are stale, as rtpbr_denoise does, and
 *   allocates M and s (both zeroed, as the first rtpbr_noise_update would) when they do not exist: from then on
 *   rtpbr_write_buffer(RTPBR_BUF_IMAGE_BUFFER) re-takes s.  Per pixel p with b = image_buffer:
 *     b.w > 0 is false:     v = 0, the pixel is not counted as estimated;
 *     M.w >= 2 (temporal):  mu = M.x / M.z;  sd = sqrt(max((M.y - (M.x * M.x) / M.z) / ((M.w - 1) * M.z), 0));
 *                           hi = mu + sd; lo = max(mu - sd, 0);  hw = 0.5f * (hi / (1 + hi) - lo / (1 + lo));
 *                           v = max(hw * hw, 0)   [fmaxf: NaN gives 0].
 *                           With s2 the per-sample variance of the batch-mean luminance, sum c_k (L_k - mu)^2 has expectation
 *                           (K - 1) s2, so sd^2 estimates the variance of the mean of M.z samples; the displayed value is
 *                           r(mean), so sd is carried through r by its two sigma points: for small sd this is r'(mu)^2 sd^2,
 *                           and v <= 1/4 whatever a firefly does to the moments.  (Moments of lum(r(batch mean)) measure the
 *                           mean of compressed batch means instead, which one bright sample moves by 1/K while it saturates
 *                           the display: 12 times too little variance at 8 x 4 spp on Cornell v3)
 *     otherwise (spatial):  over q = p + (dx, dy), dy = -3..3 (outer), dx = -3..3 (inner), inside the frame, with
 *                           RTPBR_BUF_FEAT_OBJECT equal to p's and b_q.w > 0:  L = lum(r((b_q.x / b_q.w, b_q.y / b_q.w,
 *                           b_q.z / b_q.w))); n = n + 1; s1 = s1 + L; s2 = s2 + L * L;
 *                           v = n >= 2 ? max((s2 - (s1 * s1) / n) / (n - 1), 0) : 0.
 *   With rtpbr_set_noise_estimator's pool_batches > 0 the temporal branch changes for the young pixels, M.w < pool_batches
 *   (compared as f32; b.w > 0 and M.w >= 2 as above), R = pool_radius:
 *     own = max((M.y - (M.x * M.x) / M.z) / ((M.w - 1) * M.z), 0)                 (the argument of the sqrt above)
 *     SS = 0; DF = 0; over q = p + (dx, dy), dy = -R..R (outer), dx = -R..R (inner), centre included, inside the frame, with
 *     RTPBR_BUF_FEAT_OBJECT equal to p's, b_q.w > 0 and M_q.w >= 2:
 *         SS = SS + max(M_q.y - (M_q.x * M_q.x) / M_q.z, 0);   DF = DF + (M_q.w - 1);
 *     pooled = SS / (DF * M.z)                                                   (DF >= 1: the centre qualifies)
 *     sd = sqrt(max(own, pooled))   [fmaxf];  mu, hi, lo, hw and v exactly as above.
 *   SS / DF is the pooled within-pixel estimate of the per-sample variance: differences between the neighbours' means do not
 *   enter it.  A pixel whose own batches agree by chance inherits the spread of the neighbours that did catch the light; the
 *   max keeps a noisy pixel at least as noisy as without pooling.  Pixels with M.w >= pool_batches, the spatial branch and
 *   pixels without samples are untouched, and with pool_batches = 0 every value is bit for bit what it is without the setting.
 *   pixels_estimated counts the pixels with b.w > 0, pixels_above those of them with sqrt(v) > threshold, max_noise is the
 *   largest sqrt(v) (integer atomics, and an unsigned atomic maximum over the bit patterns, which order like the values
 *   because they are >= +0: the three are independent of the order of execution).
 *
 * rtpbr_denoise_guided writes RTPBR_BUF_DENOISED_PIXELS like rtpbr_denoise (and RTPBR_BUF_NOISE: the estimate above is
 *   recomputed by every call with iterations > 0 — image_buffer has writers the library does not see, and the pass is cheap).
 *   The same taps, skip rules, tap order, normal and depth terms, average / demodulation / remodulation / tone map as
 *   rtpbr_denoise.  Beside its colour every pixel carries a variance, v_0 = v above (so v_0 follows
 *   rtpbr_set_noise_estimator's pooling).  Level k, pixel p with samples:
 *     g = sum K v_q / sum K over q = p + (dx, dy), dy = -1..1 (outer), dx = -1..1 (inner; stride 1 at every level), inside the
 *       frame, with samples and on p's object; K = {1, 2, 1; 2, 4, 2; 1, 2, 1}; both sums in tap order;
 *     ic_p = 1 / ((sigma_color * sigma_color) * max(g, variance_floor))    (no 4^k schedule);
 *     e = ((|r(c_p) - r(c_q)|^2 ic_p + |n_p - n_q|^2 in) + ((z_p - z_q) / max(z_p, 1e-6f))^2 iz);  w = h exp(-min(e, 80));
 *     c_p <- sum w c_q / sum w;  v_p <- sum (w * w) v_q / ((sum w) * (sum w)), all sums in tap order.
 *   iterations = 0 is rtpbr_denoise's iterations = 0: no estimate is made, RTPBR_BUF_NOISE and M are neither written nor
 *   allocated.  With demodulate = 1 the colours are compared demodulated while v stays
 *   the variance of the modulated luminance (the albedo is constant per object, so this rescales sigma_color per object).
 *
 * rtpbr_reproject with moments (they exist): M is gathered with exactly the accepted taps and weights of the image,
 *   SM = SM + w * M_q per component in tap order, M = SM / Wt; when the cap applies (b.w > max_history before scaling, f =
 *   max_history / b.w, the image's quotient): M.x, M.y, M.z are multiplied by f and M.w = M.w > 1 ? 1 + (M.w - 1) * f : M.w,
 *   which leaves s2 unchanged; no accepted tap: M = 0.  The snapshot becomes the warped image_buffer.  image_buffer,
 *   RTPBR_BUF_MOTION and the features are bit for bit what they are without moments.
 *
 * rtpbr_set_noise_estimator sets the estimator of rtpbr_noise_estimate, rtpbr_select_noisy and rtpbr_denoise_guided (they share
 *   one estimate pass); e == NULL restores the defaults, which are off.  Valid any time after rtpbr_create; plain context
 *   state: it survives rtpbr_refresh, rtpbr_set_config, rtpbr_set_scene and rtpbr_reproject, allocates nothing and enqueues
 *   nothing.  RTPBR_EINVAL for a NULL context or a field outside its range (pool_radius is checked even with pooling off).
 *
 * rtpbr_set_noise_tracking(RTPBR_NOISE_TRACK_SAMPLES) makes every sample a batch of its own: while the mode is on, rtpbr_sample(n)
 *   and rtpbr_sample_selected(n) of the complete-path form fold every staged sample into M inside the pass that adds it to
 *   image_buffer.  For a pixel that receives samples, with c = (r, g, b) each of its records in sample order:
 *     L = (0.299f * c.x + 0.587f * c.y) + 0.114f * c.z;
 *     M.x = M.x + L;  M.y = M.y + L * L;  M.z = M.z + 1;  M.w = M.w + 1;
 *     b.x += c.x; b.y += c.y; b.z += c.z; b.w += 1;                              (rtpbr_sample's own sum, unchanged)
 *   and after the pixel's last record of a sub-launch s = b.  This is rtpbr_noise_update's rule for cnt = 1, the batch mean being
 *   the sample itself (1 * L = L exactly); the pass overwrites s without reading it.  Pixels that receive no samples (unselected
 *   ones) keep M and s bit for bit.  So n spp give n - 1 degrees of freedom per pixel instead of (calls - 1), the estimate is
 *   valid after the first call, and "batches" in pool_batches, M.w and everything above means samples: rtpbr_noise_estimate,
 *   rtpbr_select_noisy, rtpbr_denoise_guided, the pooling and the moment warp of rtpbr_reproject / rtpbr_reproject_scene read the
 *   same buffer by the same rules.  A tracked call allocates M and s (zeroed) when they do not exist, is ordered behind
 *   asynchronous reads of the moments, and keeps item-linear staging whatever option stage_dense says (same bits, as
 *   rtpbr_sample_selected).  image_buffer, the work counters, sample_base, the timing and every other buffer are bit for bit those
 *   of the untracked call, and the result does not depend on how the staging budget splits the call into sub-launches (it
 *   splits along samples).  An rtpbr_noise_update after a tracked call finds d = 0 and changes nothing: the two may be mixed.
 *   The set call with RTPBR_NOISE_TRACK_SAMPLES first does exactly what rtpbr_noise_update does (same refusals: everything
 *   deposited so far is one batch, s = image_buffer), then sets the mode; with RTPBR_NOISE_TRACK_OFF it sets the mode and does
 *   nothing else.  The mode is plain context state: it survives rtpbr_refresh (which zeroes M and s as before), rtpbr_set_config
 *   (a new resolution frees M and s; the next tracked call makes them again), rtpbr_set_scene and rtpbr_reproject*.
 *   While the mode is on rtpbr_sample / rtpbr_sample_selected are refused with RTPBR_ESTATE, changing nothing, in the
 *   persistent-ray form (no per-sample records), with option precision = 1 (its unstaged instance keeps no records) and with
 *   tiles of world > 1.  RTPBR_EINVAL for a NULL context or another mode.
 *
 * Errors: RTPBR_ESTATE before set_config (estimate / guided: set_scene and set_camera too) and with tiles of world > 1;
 * RTPBR_EINVAL for a NULL context, a threshold that is not >= 0, iterations outside 0..8, demodulate not 0/1, a sigma or
 * variance_floor that is not finite and > 0, or whose 1/sigma^2 or 1/(sigma_color^2 variance_floor) overflows.  A refused call
 * changes nothing. */
typedef struct rtpbr_noise_stats {   /* 4-byte members, no padding */
    uint32_t pixels_estimated;   /* pixels with samples                          */
    uint32_t pixels_above;       /* ... whose noise exceeds the threshold        */
    float    max_noise;          /* the largest value of RTPBR_BUF_NOISE         */
} rtpbr_noise_stats;
typedef struct rtpbr_denoise_guided_params {   /* 4-byte members, no padding */
    int32_t iterations;      /* a-trous levels 0..8, step 2^k; 0 = tone map only                           */
    int32_t demodulate;      /* 1: filter radiance / max(albedo, 1e-3), multiply back                      */
    float   sigma_color;     /* colour distance in standard deviations of the centre's luminance           */
    float   sigma_normal, sigma_depth;
    float   variance_floor;  /* lower bound of the filtered variance in the colour term (> 0)              */
} rtpbr_denoise_guided_params;
/* Defaults (p == NULL): the best worst case of the 40 settings of examples/noise_guided.py --sweep on the two still frames of
 * section 6b (0.329 x / 0.290 x the noisy frame's display RMSE; rtpbr_denoise's defaults score 0.235 / 0.279 there: at two batches
 * of 2 spp the estimate has one degree of freedom per pixel and the plain filter is the better one — DESIGN.md section 6d).  raytracingpbr_amd.dataclass.DenoiseGuidedParams.DEFAULTS mirrors them (tests/test_noise_ref.py checks). */
#define RTPBR_DENOISE_GUIDED_DEFAULT_ITERATIONS     4
#define RTPBR_DENOISE_GUIDED_DEFAULT_DEMODULATE     0
#define RTPBR_DENOISE_GUIDED_DEFAULT_SIGMA_COLOR    16.0f
#define RTPBR_DENOISE_GUIDED_DEFAULT_SIGMA_NORMAL   0.3f
#define RTPBR_DENOISE_GUIDED_DEFAULT_SIGMA_DEPTH    0.2f
#define RTPBR_DENOISE_GUIDED_DEFAULT_VARIANCE_FLOOR 1e-3f
typedef struct rtpbr_noise_estimator {   /* 4-byte members, no padding */
    int32_t pool_batches;   /* 0 = off.  3..64: pixels with 2 <= M.w < pool_batches take max(own, pooled) */
    int32_t pool_radius;    /* 1..3: Chebyshev radius of the pooling window */
    int32_t min_samples;    /* 0 = off.  1..16777216: rtpbr_select_noisy also selects pixels with b.w < min_samples */
} rtpbr_noise_estimator;
/* Defaults (e == NULL): off.  raytracingpbr_amd.dataclass.NoiseEstimator.DEFAULTS mirrors them (tests/test_pool_ref.py checks). */
#define RTPBR_NOISE_ESTIMATOR_DEFAULT_POOL_BATCHES 0
#define RTPBR_NOISE_ESTIMATOR_DEFAULT_POOL_RADIUS  3
#define RTPBR_NOISE_ESTIMATOR_DEFAULT_MIN_SAMPLES  0
int rtpbr_noise_update(rtpbr_ctx* ctx);
int rtpbr_noise_estimate(rtpbr_ctx* ctx, float threshold, rtpbr_noise_stats* out);
int rtpbr_denoise_guided(rtpbr_ctx* ctx, const rtpbr_denoise_guided_params* p);
int rtpbr_set_noise_estimator(rtpbr_ctx* ctx, const rtpbr_noise_estimator* e);   /* NULL = the defaults */
enum { RTPBR_NOISE_TRACK_OFF = 0,       /* a batch is what rtpbr_noise_update finds deposited since the last one (the default) */
       RTPBR_NOISE_TRACK_SAMPLES = 1 }; /* complete-path form: every sample is a batch, folded in by rtpbr_sample itself      */
int rtpbr_set_noise_tracking(rtpbr_ctx* ctx, int mode);

/* ---- Adaptive sampling of the complete-path form: select pixels, then trace samples through the selected pixels only.
 *
 * Both select calls write RTPBR_BUF_SELECTION (one byte per pixel, 0 / 1) and build, on the device, the list of the selected
 * pixels in ascending buffer index x * H + y; its length comes back through n_selected (4 bytes are all that cross to the host).
 * They block.  The selection stays until the next select call; rtpbr_set_config with a new resolution frees the buffer and drops it.
 *
 * rtpbr_select_mask takes a host mask in the field layout ([x][y], y fastest), nbytes = W * H; nonzero = selected: the
 *   region-of-interest entry.
 * rtpbr_select_noisy recomputes the noise estimate exactly as rtpbr_noise_estimate(threshold) does (features rendered first when
 *   stale; writes RTPBR_BUF_NOISE), then selects pixel p when
 *     image_buffer[p].w > 0 is false (no samples: for example no history after rtpbr_reproject), or
 *     some pixel q inside the frame with max(|dx|, |dy|) <= dilate has noise[q] > threshold          (dilate 0..3), or
 *     image_buffer[p].w < (float)min_samples                   (rtpbr_set_noise_estimator; min_samples = 0: never).
 *   Comparisons only, no arithmetic.  dilate > 0 keeps the neighbours of a noisy pixel sampling: the mitigation of the bias of
 *   stopping a pixel on an estimate made from its own samples.
 *
 * rtpbr_sample_selected is rtpbr_sample(n) restricted to the list: every selected pixel receives the samples with absolute
 *   indices sample_base .. sample_base + n - 1, added in sample order; every other pixel of image_buffer stays as it is, bit for
 *   bit; sample_base advances by n (unselected pixels skip those indices, so a pixel's sample k is the same ray whatever the
 *   selection history was).  An empty selection traces nothing and still advances sample_base; a full one gives the image_buffer
 *   and the work counters of rtpbr_sample(n).  Counters: samples = deposits = n_selected * n.  Asynchronous, ordered behind
 *   asynchronous reads, flushes lazy shading and is timed (rtpbr_last_sample_ms) like rtpbr_sample.  It runs the general
 *   ahead-of-time kernels with item-linear staging whatever the scheduler, jit, jit_bake, primary_split and stage_dense options
 *   say: same bits.
 *
 * Errors: RTPBR_ESTATE before set_config / set_scene / set_camera and with tiles of world > 1; rtpbr_sample_selected also before
 * any select call, in the persistent-ray form (it has cfg.adaptive_sampling) and with option precision = 1.  RTPBR_EINVAL for
 * NULL pointers, nbytes != W * H, n < 0, a threshold that is not >= 0, dilate outside 0..3.  A refused call changes nothing.
 *
 * Tiers: a share of the batch per pixel.  rtpbr_set_option "select_tiers" = T (1..8, default 1: everything above) and
 *   "select_batch" = B (1..65536, default 16: the n the host will pass to rtpbr_sample_selected) are read by the select calls
 *   (rtpbr_select_mask, rtpbr_select_noisy, rtpbr_select_error, rtpbr_select_blend_error) and by nothing else: a selection keeps
 *   the tiers it was built with, changing either option afterwards does not alter it, and rtpbr_sample_selected reads neither.
 *   With T > 1 every selected pixel p has a tier t in 0 .. T - 1; tier 0 is the full share.  Membership is the rule above, unchanged.
 *     rtpbr_select_mask: byte b = 0: not selected; b >= 1: t = min(b, T) - 1 (1 = the full share, 2 = half of it, ...).
 *     rtpbr_select_noisy / rtpbr_select_error / rtpbr_select_blend_error: a pixel selected because it has no samples, fewer than
 *       min_samples or (the error rules) an empty half: t = 0.  Otherwise, with `plane` the call's plane (noise, denoised error,
 *       blend error) and b = image_buffer[p], in f32, every operation exactly rounded, nothing contracted:
 *         m    = fmaxf over the pixels q inside the frame with max(|dx|, |dy|) <= dilate and plane[q] > threshold, of plane[q]
 *                (p is selected by the plane, so there is at least one)
 *         r    = m / threshold
 *         need = b.w * (r * r - 1.0f)
 *         t    = the number of k in 1 .. T - 1 with need <= (float)max(1, B >> k)
 *       The bounds fall with k, so the comparisons that hold are a prefix: t is the smallest share that covers `need`.  A NaN or
 *       infinite `need` (threshold = 0, an infinite plane value) satisfies none: t = 0.  Reading: the plane is the standard
 *       deviation of a mean of b.w samples, so `need` is how many more samples bring it to the threshold.  The window maximum
 *       keeps dilate's mitigation: a quiet pixel beside a noisy one takes the noisy one's tier.
 *   RTPBR_BUF_SELECTION holds 0 or 1 + t.  The list is ordered by tier, then by ascending buffer index within a tier; n_selected
 *   is the total over all tiers.  rtpbr_get_counter "select_tier0" .. "select_tier7": the pixels in that tier of the current
 *   selection (0 for tiers >= T and before any selection; with T = 1 select_tier0 = n_selected), answered from the host without a
 *   synchronisation.
 *   rtpbr_sample_selected(n) on a tiered selection: with the shares s_t = max(1, n >> t) for n >= 1 (s_T = 0), a pixel of tier t
 *   receives the samples with absolute indices sample_base .. sample_base + s_t - 1, added in sample order, and skips the
 *   indices up to sample_base + n - 1; sample_base advances by n, so a pixel's sample k is still the same ray whatever was
 *   selected.  n = 0 traces nothing.  It runs as stages t = T - 1 .. 0, stage t tracing the indices sample_base + s_{t+1} ..
 *   sample_base + s_t - 1 through the pixels of tiers 0 .. t (a prefix of the list), each an ordinary selected launch; stages with
 *   s_t = s_{t+1} or no pixels are skipped.  Counters: samples = deposits = the sum over t of (pixels in tier t) * s_t;
 *   rtpbr_last_sample_ms sums all stages and counts all their sub-launches.  Noise tracking, per-sample halves and every refusal
 *   are those of the plain selected launch.
 *
 * Lattices built on the device: rtpbr_set_option "select_lattice" = px + 16 * py + 256 * phx + 4096 * phy is a command spelled as
 *   an option (as "reserve_spp" is).  With 1 <= px, py <= 8, 0 <= phx < px, 0 <= phy < py and no other bits set it leaves the
 *   context exactly as rtpbr_select_mask leaves it for the mask "x % px == phx && y % py == phy" (bytes 0 / 1): the same
 *   RTPBR_BUF_SELECTION, the same n_selected = nx * ny with nx = phx < W ? (W - phx + px - 1) / px : 0 and ny likewise (the host
 *   computes it the same way: nothing comes back), every lattice pixel in tier 0 of the current "select_tiers", the same
 *   counters "select_tier*", and every later call answers as after that rtpbr_select_mask, bit for bit.  The call enqueues ONE
 *   kernel and returns: no mask crosses to the device, nothing is counted or scanned, nothing blocks; it is ordered behind
 *   asynchronous reads of RTPBR_BUF_SELECTION.  The list is in ascending buffer index, as rtpbr_select_mask's is (a build with
 *   -DRT_LATTICE_ORDER=1 orders it in blocks of 8 x 8 lattice pixels instead; the order is not observable: a pixel's sample k is
 *   the same ray wherever the pixel stands in the list).
 *   Value 0 is accepted and does nothing (rtpbr_jit_prebuild option strings may carry it).  Every other value is refused with
 *   RTPBR_EINVAL and RTPBR_SELECT_LATTICE_REFUSAL; a lattice is then refused as rtpbr_select_mask refuses, in its order and words:
 *   RTPBR_ESTATE before set_config / set_scene / set_camera (and on a context without a device), RTPBR_ESTATE with tiles of
 *   world > 1.  A refused call changes nothing. */
#define RTPBR_SELECT_LATTICE_REFUSAL \
    "select_lattice must be 0 (nothing) or px + 16 * py + 256 * phx + 4096 * phy with 1 <= px, py <= 8, 0 <= phx < px and 0 <= phy < py"
int rtpbr_select_mask(rtpbr_ctx* ctx, const uint8_t* mask, size_t nbytes, uint32_t* n_selected);
int rtpbr_select_noisy(rtpbr_ctx* ctx, float threshold, int dilate, uint32_t* n_selected);
int rtpbr_sample_selected(rtpbr_ctx* ctx, int n);

/* ---- The error of the DENOISED frame from two half buffers, and sampling driven by it.
 *
 * rtpbr_noise_estimate and rtpbr_select_noisy describe the raw average in image_buffer; a host that displays
 * RTPBR_BUF_DENOISED_PIXELS would sample on long after that picture stopped changing.  Here the samples are kept in two
 * independent halves A and B, both are filtered exactly as rtpbr_denoise filters image_buffer, and the difference of the two
 * results measures the variance of the filtered full frame — correlations between neighbours included, whatever the filter does.
 * IT MEASURES VARIANCE ONLY: the filter's bias (blur inside one object) is the same in both halves and no difference of them
 * sees it.  The estimate answers "has the denoised picture stopped moving", not "is it right" (on Cornell
 * v3 the denoised frame's error against the converged frame stops falling near 0.066 while the estimate goes to 0).
 * lum(c) = (0.299f * c.x + 0.587f * c.y) + 0.114f * c.z as in the noise section; every operation is f32, nothing fused.
 *
 * rtpbr_half_update deals what was deposited into image_buffer since the last update to one half.  Half A is stored
 *   (RTPBR_BUF_HALF_BUFFER); half B never is: it is image_buffer - A per component.  A and an internal snapshot sh are allocated
 *   zeroed on the first call, so everything accumulated until then is the first batch.  Per pixel, with b = image_buffer:
 *     d = b - sh per component;
 *     if d.w > 0: cB = sh.w - A.w; if A.w <= cB then A = A + d per component (otherwise the batch stays in B);
 *     sh = b in every case.
 *   The half with fewer samples takes the batch, so equal batches alternate A, B, A, ... per pixel, and a pixel
 *   rtpbr_sample_selected skipped keeps its bits.  Like rtpbr_noise_update the call flushes lazy shading, is ordered behind
 *   asynchronous reads of RTPBR_BUF_HALF_BUFFER, is asynchronous and writes nothing else; it is independent of the moments and
 *   their snapshot.  Once A exists: rtpbr_refresh zeroes A and sh; rtpbr_write_buffer(RTPBR_BUF_IMAGE_BUFFER) zeroes A and sets
 *   sh to the written data (written data is no batch: it lies in B); rtpbr_reproject and rtpbr_reproject_scene zero A after the
 *   gather and set sh to the warped image_buffer (the history is one body of samples: it lies in B; A is not warped unless
 *   rtpbr_set_half_mode turned warp on, see below).  Until
 *   their next batch such pixels have an empty half and count as not estimated below.  rtpbr_set_config with a new resolution
 *   frees both buffers.  image_buffer, the motion buffer, the moments and the features are bit for bit what they are without.
 *   Errors: RTPBR_EINVAL for NULL; RTPBR_ESTATE before rtpbr_set_config and with tiles of world > 1.
 *
 * rtpbr_denoise_error writes RTPBR_BUF_DENOISED_ERROR and, if out != NULL, the statistics; it blocks like rtpbr_noise_estimate.
 *   p == NULL: rtpbr_denoise's defaults; e == NULL: radius = RTPBR_ERROR_DEFAULT_RADIUS.  In order: lazy shading is flushed, the
 *   call is ordered behind asynchronous reads of the error buffer, the features are rendered if stale; DA = rtpbr_denoise's
 *   filter with p applied to A in place of image_buffer, DB = the same applied to B = image_buffer - A (materialised per
 *   component), "has samples" meaning that buffer's own count > 0 in either run.  RTPBR_BUF_DENOISED_PIXELS, image_buffer, the
 *   moments, RTPBR_BUF_NOISE and the work counters are untouched.  Per pixel q, cA = A.w, cB = image_buffer.w - A.w:
 *     q is valid when cA > 0 and cB > 0;
 *     dl = lum(DA_q) - lum(DB_q);   e_q = fmaxf((dl * dl) * ((cA * cB) / ((cA + cB) * (cA + cB))), 0)   (a NaN gives 0).
 *   (With s2 the per-sample variance of the filtered value E[(DA - DB)^2] = s2 (1/cA + 1/cB) and the full frame's variance is
 *   s2 / (cA + cB): hence the factor, 1/4 for equal halves.)  Per pixel p: S = 0, n = 0; over q = p + (dx, dy), dy = -R..R
 *   (outer), dx = -R..R (inner), inside the frame, on p's RTPBR_BUF_FEAT_OBJECT, valid: S = S + e_q, n = n + 1;
 *     error_p = sqrt(S / n), correctly rounded, when p itself is valid; otherwise error_p = 0 and p is not estimated.
 *   One degree of freedom per pixel, averaged over the window: calibrated within 0.9 .. 1.2 of the empirical variance of the
 *   denoised luminance on Cornell v3.  pixels_estimated counts the valid pixels, pixels_above those with
 *   error > threshold, max_noise is the largest value.
 *   Errors: RTPBR_EINVAL for a NULL context, parameters rtpbr_denoise refuses, a radius outside 1..3, a threshold that is not
 *   >= 0; RTPBR_ESTATE before set_config / set_scene / set_camera, with tiles of world > 1 and before the first rtpbr_half_update.
 *
 * rtpbr_select_error is rtpbr_select_noisy's counterpart: same list order, same blocking, same RTPBR_BUF_SELECTION.  It reads
 *   RTPBR_BUF_DENOISED_ERROR as the last rtpbr_denoise_error wrote it (it does not recompute it: that costs two filter runs) and
 *   selects pixel p when, with the current buffer contents,
 *     image_buffer[p].w > 0 is false, or
 *     A[p].w > 0 is false, or image_buffer[p].w - A[p].w > 0 is false (a half is empty), or
 *     some pixel q inside the frame with max(|dx|, |dy|) <= dilate has error[q] > threshold          (dilate 0..3), or
 *     image_buffer[p].w < (float)min_samples                   (rtpbr_set_noise_estimator).
 *   Errors as rtpbr_select_noisy, and RTPBR_ESTATE before the first rtpbr_denoise_error.
 * A refused call changes nothing. */
typedef struct rtpbr_error_params {   /* 4-byte members, no padding */
    int32_t radius;        /* 1..3: the window of the error estimate is (2 radius + 1)^2 */
} rtpbr_error_params;
/* Default (e == NULL): the 5x5 window of the calibration in DESIGN.md section 6j.
 * raytracingpbr_amd.dataclass.ErrorParams.DEFAULTS mirrors it (tests/test_half_ref.py checks). */
#define RTPBR_ERROR_DEFAULT_RADIUS 2
int rtpbr_half_update(rtpbr_ctx* ctx);
int rtpbr_denoise_error(rtpbr_ctx* ctx, const rtpbr_denoise_params* p, const rtpbr_error_params* e, float threshold, rtpbr_noise_stats* out);
int rtpbr_select_error(rtpbr_ctx* ctx, float threshold, int dilate, uint32_t* n_selected);

/* ---- The bias-aware blend of the denoised and the raw frame, from the same two halves.
 *
 * rtpbr_denoise_error sees variance only.  What the a-trous filter leaves behind once the noise is gone is bias — blur inside one
 * object — and a host that shows RTPBR_BUF_DENOISED_PIXELS never converges, while the raw average does.  The two halves hold what
 * is needed to see that bias: for one half, filter(half) - raw(half) estimates bias - noise of that half, the two halves' noise is
 * independent, so the PRODUCT of the two differences has expectation bias^2, and the covariance of the raw frame with
 * (filtered - raw) gives the mean-square-optimal weight between the two frames.  rtpbr_denoise_blend is a member of the denoise
 * family: it writes RTPBR_BUF_DENOISED_PIXELS as rtpbr_denoise_guided does (so rtpbr_present(RTPBR_PRESENT_DENOISED) and every
 * read of that buffer serve the blended frame), and RTPBR_BUF_BLEND_WEIGHT, and nothing else: image_buffer, half A and its
 * snapshot, the moments, RTPBR_BUF_NOISE, RTPBR_BUF_DENOISED_ERROR, the selection and the work counters keep their bits.  It
 * blocks like rtpbr_denoise_error (the statistics come back), flushes lazy shading, is ordered behind asynchronous reads of the
 * two buffers it writes and renders stale features first.  p == NULL: rtpbr_denoise's defaults; e == NULL: the defaults below.
 *
 * Every operation is f32, in the order written, nothing fused; lum is the noise section's.  The statistics are taken on LINEAR
 * radiance, before the tone map (in display space the tone map saturates and the raw half is no longer unbiased).  With
 * b = image_buffer and A = half A:
 *   B = b - A per component (materialised as for rtpbr_denoise_error);
 *   F(buf) = rtpbr_denoise's filter with p applied to buf, "has samples" meaning buf's own count > 0, stopped before the tone map:
 *     the linear colour after remodulation, exactly the value the last level hands to the tone map;
 *   FD = F(b), FA = F(A), FB = F(B);   Pb = (b.x / b.w, b.y / b.w, b.z / b.w), PA and PB alike from A and B;
 *   m = (float)min_half_samples, z2 = z * z.
 * Per pixel q, cA = A.w, cB = B.w (= b.w - A.w):
 *   q is usable when cA >= m and cB >= m;
 *   f  = (cA * cB) / ((cA + cB) * (cA + cB));
 *   dA = lum(FA) - lum(PA);  dB = lum(FB) - lum(PB);  dp = lum(PA) - lum(PB);  dd = dA - dB;  dl = lum(FD) - lum(Pb);
 *   a_q = (f * dp) * dd;     q_q = dl * dl;     x_q = dA * dB.
 * Per usable pixel p, all sums from +0, over q = p + (dx, dy), dy = -R..R (outer), dx = -R..R (inner), inside the frame, on p's
 * RTPBR_BUF_FEAT_OBJECT, usable:
 *   n = n + 1;  SC = SC + a_q;  SQ = SQ + q_q;  SX = SX + x_q;  SXX = SXX + x_q * x_q;
 *   m1 = SX / n;   v = fmaxf(SXX / n - m1 * m1, 0);
 *   significant = m1 > 0 and (m1 * m1) * n > z2 * v;
 *   t = 1 unless significant; otherwise t = -SC / SQ; if (!(t < 1)) t = 1; if (t < 0) t = 0          (a NaN gives 1).
 * A pixel that is not usable has t = 1.  RTPBR_BUF_BLEND_WEIGHT = t.  For a pixel with b.w > 0:
 *   t == 1: c = FD;   otherwise u = 1 - t; c.k = FD.k + u * (Pb.k - FD.k) per channel;   denoised = tone_map(cfg, (c, 1));
 * a pixel without samples shows what rtpbr_post_process shows, and its weight is 1.
 * Why this shape: with raw = truth + noise and filtered = truth + bias + noise', the weight t on the filtered colour that
 * minimises E[(t filtered + (1 - t) raw - truth)^2] is -cov(raw, filtered - raw) / E[(filtered - raw)^2].  dp dd is the halves'
 * sample of that covariance — (PA - PB) carries the raw noise, (dA - dB) the noise of filtered - raw, the truth and the bias
 * cancel in both — and f scales a difference of halves to the full frame as in the error section: E[SC / n] = cov, SQ / n
 * estimates E[(filtered - raw)^2].  SX / n estimates bias^2; its standard error is sqrt(v / n), from SXX; the gate "the squared
 * bias exceeds z standard errors" is written without a root.  Without the gate the weight lets raw noise back in where the halves
 * cannot see any bias yet.  With t = 1 everywhere — min_half_samples above every count, or no significant
 * window — the call writes rtpbr_denoise(p)'s bytes exactly.
 * Statistics: pixels_estimated = the usable pixels, pixels_above = those with t < 1, max_noise = the largest 1 - t.
 * Errors, each before anything changes: RTPBR_EINVAL for a NULL context, parameters rtpbr_denoise refuses, a radius outside 1..3,
 * a z that is not finite and >= 0, min_half_samples outside 1..16777216; RTPBR_ESTATE before set_config / set_scene / set_camera,
 * with tiles of world > 1 and before half A exists (no rtpbr_half_update or dealing call yet). */
typedef struct rtpbr_blend_params {   /* 4-byte members, no padding */
    int32_t radius;             /* 1..3: window (2 radius + 1)^2 on the pixel's object      */
    float   z;                  /* >= 0, finite: the bias must exceed z standard errors     */
    int32_t min_half_samples;   /* 1..16777216: both halves need this many samples          */
} rtpbr_blend_params;
/* Defaults (e == NULL): the setting measured in DESIGN.md section 6l.
 * raytracingpbr_amd.dataclass.BlendParams.DEFAULTS mirrors them (tests/test_blend_ref.py checks). */
#define RTPBR_BLEND_DEFAULT_RADIUS 3
#define RTPBR_BLEND_DEFAULT_Z 2.0f
#define RTPBR_BLEND_DEFAULT_MIN_HALF_SAMPLES 16
int rtpbr_denoise_blend(rtpbr_ctx* ctx, const rtpbr_denoise_params* p, const rtpbr_blend_params* e, rtpbr_noise_stats* out);

/* ---- The same blend across the a-trous levels: narrow the filter where the halves see bias.
 *
 * rtpbr_denoise_blend repairs the filter's bias by giving way to the RAW average, so it hands back the noise reduction wherever it
 * acts.  The a-trous filter already computes a ladder of narrower filters: level k's intermediate result is the filter with
 * iterations = k, because the schedule ic_k = ic_0 4^k does not depend on the level count.  rtpbr_denoise_blend_levels judges every
 * rung of that ladder with the blend's statistics, the finer level k - 1 standing where the blend has the raw average, and keeps
 * of each level's increment the fraction the halves vouch for.  It is a member of the denoise family with the blend's state rules
 * word for word: it writes RTPBR_BUF_DENOISED_PIXELS (rtpbr_present(RTPBR_PRESENT_DENOISED) and every read of that buffer serve
 * its frame), RTPBR_BUF_BLEND_WEIGHT and RTPBR_BUF_BLEND_DEPTH, and nothing else; it blocks, flushes lazy shading, is ordered
 * behind asynchronous reads of the three buffers it writes and renders stale features first.  p == NULL: rtpbr_denoise's defaults;
 * e == NULL: RTPBR_BLEND_DEFAULT_* (the blend's struct, range checks and defaults).  rtpbr_denoise_blend keeps its behaviour and
 * its bits.
 *
 * Every operation is f32, in the order written, nothing fused.  b, A, B, lum, m, z2, "usable" and f are the blend section's.
 *   K = p->iterations;
 *   F_k(buf), k = 0..K: rtpbr_denoise's filter with iterations = k and p's other fields applied to buf, "has samples" meaning buf's
 *     own count > 0, stopped before the tone map — the blend section's F for iterations = k (+0 for a pixel without samples).
 *     k = 0 is the average, demodulated and remodulated when p->demodulate is set; with demodulate the remodulation
 *     c * max(albedo, 1e-3) is applied at every k, as the last level applies it;
 *   FD_k = F_k(b), FA_k = F_k(A), FB_k = F_k(B).
 * For each level k = 1..K, per usable pixel q (f from cA, cB as in the blend section):
 *   dA = lum(FA_k) - lum(FA_{k-1});  dB = lum(FB_k) - lum(FB_{k-1});  dp = lum(FA_{k-1}) - lum(FB_{k-1});
 *   dd = dA - dB;  dl = lum(FD_k) - lum(FD_{k-1});   a_q = (f * dp) * dd;  q_q = dl * dl;  x_q = dA * dB.
 * Per usable pixel p: the blend's window and tap order, its sums n, SC, SQ, SX, SXX from +0, its m1, v, gate and clamp give t_k
 * (1 unless significant; a NaN gives 1).  A pixel that is not usable has t_k = 1 for every k.  Then, for a pixel with b.w > 0:
 *   T_0 = 1;  T_k = T_{k-1} * t_k;  depth = 0;  c = FD_0;
 *   k = 1..K in order:  depth = depth + T_k;   c.ch = c.ch + T_k * (FD_k.ch - FD_{k-1}.ch)  per channel;
 *   if T_K == 1: c = FD_K   (every t_k was 1: the bytes are then rtpbr_denoise(p)'s);
 *   denoised = tone_map(cfg, (c, 1)).
 * Once a fine level is refused every coarser increment is scaled down with it: a coarser level is not trusted past a finer one the
 * halves have caught blurring.  RTPBR_BUF_BLEND_WEIGHT = T_K; RTPBR_BUF_BLEND_DEPTH = depth, in 0..K.  A pixel without samples
 * shows what rtpbr_post_process shows; its weight is 1 and its depth K.  K = 0 writes rtpbr_denoise's bytes, weight 1, depth 0.
 * Statistics: pixels_estimated = the usable pixels, pixels_above = those with T_K < 1, max_noise = the largest 1 - T_K.
 * Memory: beside the two outputs the call keeps the records of levels k - 1 and k of all three filter runs, six (W,H) planes of
 * 16 bytes (199 MB at 1920 x 1080), allocated by the first call and freed, like both outputs, by rtpbr_set_config with a new
 * resolution.
 * Errors, each before anything changes: exactly rtpbr_denoise_blend's. */
int rtpbr_denoise_blend_levels(rtpbr_ctx* ctx, const rtpbr_denoise_params* p, const rtpbr_blend_params* e, rtpbr_noise_stats* out);

/* ---- The error of the LEVEL-BLENDED frame, and sampling driven by it.
 *
 * rtpbr_denoise_error measures the variance of the unblended filter and is blind to bias; a host that shows
 * rtpbr_denoise_blend_levels' frame wants to know how wrong THAT frame still is.  The two halves answer as they do for
 * rtpbr_denoise_error, but on the blended frame itself: the full frame's weights T_k applied to each half's own ladder give XA and
 * XB, the blended frame of either half; their difference measures the variance, correlations between neighbours included; the
 * product of the halves' (blended - raw) has expectation bias^2, because the halves' noise is independent (the argument
 * rtpbr_denoise_blend rests on); variance plus squared bias is the mean-square error of the picture on the screen.  THE BIAS IS
 * ONLY WHAT THE HALVES CAN SEE: averaged over the window, on the pixel's object, where both halves hold min_half_samples.
 *
 * rtpbr_blend_error does everything rtpbr_denoise_blend_levels(p, e) does — RTPBR_BUF_DENOISED_PIXELS, RTPBR_BUF_BLEND_WEIGHT and
 *   RTPBR_BUF_BLEND_DEPTH come out with the same bytes, under the same state rules (it blocks, flushes lazy shading, is ordered
 *   behind asynchronous reads of the buffers it writes, renders stale features first) — and writes RTPBR_BUF_BLEND_ERROR besides.
 *   Nothing else changes: image_buffer, half A and its snapshot, the moments, RTPBR_BUF_NOISE, RTPBR_BUF_DENOISED_ERROR, the
 *   selection and the work counters keep their bits.  NULL p, e, w: the defaults of rtpbr_denoise, rtpbr_denoise_blend and
 *   rtpbr_denoise_error.  out (if not NULL) receives the statistics of the ERROR plane, not the blend's: pixels_estimated = the
 *   valid pixels, pixels_above = those with error > threshold, max_noise = the largest error.
 *   Every operation is f32, in the order written, nothing fused.  b, A, B, cA, cB, f, lum, m, "usable", FD_k, FA_k, FB_k, T_k and K
 *   are those of the blend-levels section; PA, PB the blend section's raw averages of the halves.
 *   Per pixel (only pixels with samples in the half are ever read), alongside the ladder sum for c:
 *     XA = FA_0;  XB = FB_0;
 *     k = 1..K in order:  XA.ch = XA.ch + T_k * (FA_k.ch - FA_{k-1}.ch)  per channel;  XB likewise from FB;
 *     if T_K == 1: XA = FA_K, XB = FB_K.
 *   Variance, in display space as in rtpbr_denoise_error.  q is valid when cA > 0 and cB > 0:
 *     dl = lum(tone_map(cfg, (XA, 1))) - lum(tone_map(cfg, (XB, 1)));   e_q = fmaxf((dl * dl) * f, 0)        (a NaN gives 0).
 *   Squared bias, in linear radiance (the raw half is unbiased only there), for usable q (cA >= m and cB >= m):
 *     x_q = (lum(XA) - lum(PA)) * (lum(XB) - lum(PB));
 *   a valid pixel that is not usable has x_q = +0 and does not count in nb.
 *   Slope of the display luminance at the blended colour: c is the linear colour the call tone-maps (a pixel with b.w > 0),
 *     Y = lum(c);   c1 = (1.0625f * c.x, 1.0625f * c.y, 1.0625f * c.z);
 *     s = (lum(tone_map(cfg, (c1, 1))) - lum(tone_map(cfg, (c, 1)))) / (0.0625f * Y)  when Y > 0;   s = 0 otherwise.
 *   Per valid pixel p, over rtpbr_denoise_error's window with its tap order — q = p + (dx, dy), dy = -R..R (outer), dx = -R..R
 *   (inner), R = w->radius, inside the frame, on p's RTPBR_BUF_FEAT_OBJECT, valid — all sums from +0:
 *     S = S + e_q;  n = n + 1;  and for usable q:  SX = SX + x_q;  nb = nb + 1;
 *     bias2 = nb > 0 ? fmaxf(SX / nb, 0) : 0                                                      (a NaN gives 0);
 *     error_p = sqrt(S / n + (s * s) * bias2), correctly rounded.
 *   A pixel that is not valid has error 0 and is not estimated.
 *   With min_half_samples above every count every T_k is 1, no pixel is usable, XA = FA_K and XB = FB_K: the plane is then
 *   rtpbr_denoise_error(p, w)'s bit for bit.  K = 0 is allowed: the frame is the raw average, the variance is the raw halves' and
 *   bias2 is exactly 0 without demodulate (XA = PA; with it XA differs from PA by the rounding of c / albedo * albedo, and bias2
 *   is of that order squared).  NOT CALIBRATED: against the empirical error on Cornell v3 the mean of error^2 is 6.6 to 7.4 times
 *   too large (the bias term; the variance term alone is about half the empirical variance): DESIGN.md section 6n.
 *   Memory: beside what rtpbr_denoise_blend_levels keeps, two (W,H) planes of 16 bytes (XA, XB) and the 4-byte output plane (75 MB
 *   at 1920 x 1080), allocated by the first call and freed by rtpbr_set_config with a new resolution.
 *   Errors, each before anything changes: rtpbr_denoise_blend_levels', and rtpbr_denoise_error's for w and threshold (RTPBR_EINVAL
 *   for a window radius outside 1..3 and a threshold that is not >= 0).
 *
 * rtpbr_select_blend_error is rtpbr_select_error's rule word for word, reading RTPBR_BUF_BLEND_ERROR as the last rtpbr_blend_error
 *   wrote it in the place of RTPBR_BUF_DENOISED_ERROR.  Errors as rtpbr_select_error, and RTPBR_ESTATE before the first
 *   rtpbr_blend_error. */
int rtpbr_blend_error(rtpbr_ctx* ctx, const rtpbr_denoise_params* p, const rtpbr_blend_params* e, const rtpbr_error_params* w,
                      float threshold, rtpbr_noise_stats* out);
int rtpbr_select_blend_error(rtpbr_ctx* ctx, float threshold, int dilate, uint32_t* n_selected);

/* ---- The same estimate with the bias in display space per tap (rtpbr_blend_error_display).
 *
 * rtpbr_blend_error averages the squared bias over the window in linear radiance and converts the mean with the slope of the tone
 * map at the centre pixel.  Where the window holds a pixel whose tone map is saturated — linear luminance of tens, a slope of
 * nearly 0, a linear bias^2 of 16 to 20 on the ceiling beside Cornell's light — every neighbour inherits that bias^2 at its own
 * slope, and the estimate overstates the mean-square error about seven times.  This call converts each tap's
 * product with the TAP's own slope before it is summed.  THE NUMBER IS: the variance of the level-blended frame's display
 * luminance plus the squared DISPLAY-SPACE bias the halves can see, as a root.  The variance term is rtpbr_blend_error's and is
 * still about half the empirical variance (the halves share the weights T_k; DESIGN.md sections 6n (2), 6o and 8).
 *
 * rtpbr_blend_error_display is rtpbr_blend_error(p, e, w, threshold, out) in everything but the bias term: the same
 *   RTPBR_BUF_DENOISED_PIXELS, RTPBR_BUF_BLEND_WEIGHT and RTPBR_BUF_BLEND_DEPTH byte for byte, the same state rules, errors, NULL
 *   defaults and statistics, and the same output plane: RTPBR_BUF_BLEND_ERROR holds what the LAST of the two calls wrote, and
 *   rtpbr_select_blend_error, rtpbr_present and every read work on it unchanged.  Nothing else changes.
 *   Every operation is f32, in the order written, nothing fused.  XA, XB, PA, PB, "valid", "usable", e_q, x_q, s, the window, its tap
 *   order, S, n and nb are those of the section above.
 *   s_q is s of pixel q: defined for every pixel, 0 where b.w > 0 is false or Y > 0 is false.
 *   For usable q:
 *     xd_q = (s_q * s_q) * x_q;
 *   a valid pixel that is not usable has xd_q = +0 and does not count in nb.
 *   Per valid pixel p, all sums from +0:
 *     S = S + e_q;  n = n + 1;  and for usable q:  SX = SX + xd_q;  nb = nb + 1;
 *     bias2 = nb > 0 ? fmaxf(SX / nb, 0) : 0                                                      (a NaN gives 0);
 *     error_p = sqrt(S / n + bias2), correctly rounded.
 *   A pixel that is not valid has error 0 and is not estimated.
 *   With min_half_samples above every count the plane is rtpbr_denoise_error(p, w)'s bit for bit, and with K = 0 without demodulate
 *   it is rtpbr_blend_error's (both are then the variance alone).  Calibration on Cornell v3: DESIGN.md section 6o.
 *   Memory: beside what rtpbr_blend_error keeps, one (W,H) plane of 4 bytes for s (8 MB at 1920 x 1080): a tap's s_q cannot live in
 *   the output plane, whose words the neighbouring pixels' estimates overwrite.  Allocated by the first call and freed by
 *   rtpbr_set_config with a new resolution.
 *   Errors, each before anything changes: rtpbr_blend_error's. */
int rtpbr_blend_error_display(rtpbr_ctx* ctx, const rtpbr_denoise_params* p, const rtpbr_blend_params* e, const rtpbr_error_params* w,
                              float threshold, rtpbr_noise_stats* out);

/* ---- The level blend on the coverage-weighted filter (options "blend_coverage", "blend_coverage_grid", "blend_coverage_power",
 * "blend_coverage_resolve"; counter "blend_resolved").
 *
 * The three ladders of the three calls above are rtpbr_denoise's, which never takes a tap across object indices: a silhouette pixel
 * is pulled to its centre ray's object, the halves read that as bias, and the blend hands the pixel back to its raw average.
 * rtpbr_denoise_coverage (below) repairs exactly those pixels but is the plain filter only.  With option "blend_coverage" = 1
 * (rtpbr_set_option; 0 or 1, default 0) rtpbr_denoise_blend_levels, rtpbr_blend_error and rtpbr_blend_error_display — and only they:
 * rtpbr_denoise, rtpbr_denoise_guided, rtpbr_denoise_coverage, rtpbr_denoise_error, rtpbr_denoise_blend, rtpbr_post_process and
 * rtpbr_present never read the four options and keep their bytes, and the three calls never read "denoise_fill" or "coverage_fill" —
 * run the rule below with the rtpbr_coverage_params (grid, power, resolve) = ("blend_coverage_grid": 2 or 4, default 4;
 * "blend_coverage_power": 0..8, default 4; "blend_coverage_resolve": 0 or 1, default 1).  It applies with K = iterations > 0; with
 * iterations = 0 there is no level, the options are not read and the bytes are those of "blend_coverage" = 0.  With 0 everything
 * above holds, bit for bit.
 *   1. k_q = a_q * a_q * ... (power factors, left to right, 1.0f for power = 0), a_q = (float)n_own_q / (float)n_sub_q of the coverage
 *      plane, which the call renders first at the option's grid when it is stale (as rtpbr_denoise_coverage does; the plane lives as
 *      long as the features).
 *   2. All three chains — image_buffer, half A, half B — run rtpbr_denoise_coverage's level: rtpbr_denoise's tap loop, same inputs,
 *      same tap order, same clamp and exp, with w = (h exp(-min(e, 80))) k_q for every tap but the centre's own.  k is geometric,
 *      so the one plane serves all three chains.  F_0 .. F_K of a chain are its levels after remodulation, as above.
 *   3. The window statistics are unchanged: t_k, T_k = T_(k-1) t_k, RTPBR_BUF_BLEND_WEIGHT = T_K, RTPBR_BUF_BLEND_DEPTH = the sum of
 *      the T_k, the running colour c = F_0 + the sum of T_k (F_k - F_(k-1)), and c = F_K itself where T_K == 1 — all on these ladders.
 *   4. After the last level the blended LINEAR colour L_p = c (the value the plain rule hands to the tone map) goes to a private
 *      (W,H,3) plane; a pixel without samples (image_buffer[p].w == 0) holds +0 there.
 *   5. The resolve of rtpbr_denoise_coverage, operation for operation, with L in the place of its F and "with samples" =
 *      image_buffer[q].w > 0: if resolve and n_second_p > 0, E2 = the k-weighted 3x3 mean (weights 1/2 edge, 1/3 corner) of L over
 *      the neighbours with samples on second_object_p; if its sw > 0, L_p <- ((float)n_own L_p + (float)n_second E2) /
 *      (float)(n_own + n_second) per channel and the pixel counts as resolved.  RTPBR_BUF_DENOISED_PIXELS = the configured tone map of
 *      (L_p, 1); a pixel without samples shows what rtpbr_post_process shows, is nobody's tap and nobody's E2 neighbour, is not
 *      resolved, and has weight 1 and depth K.
 *   6. RTPBR_BUF_BLEND_ERROR (the two error calls) stays the estimate of the blended frame BEFORE the resolve: XA, XB, their four
 *      luminances and the slope s are taken at the pre-resolve colour c, exactly as above, on these ladders.  The resolve moves only
 *      two-object pixels, towards a neighbour mean the halves have no separate view of; an estimate of the resolved frame is not
 *      made.  The statistics each call returns are its own as above (of T_K, of the error plane), before the resolve.
 *   The three calls still write the same RTPBR_BUF_DENOISED_PIXELS, RTPBR_BUF_BLEND_WEIGHT and RTPBR_BUF_BLEND_DEPTH as one another.
 *   So: with "blend_coverage_power" = 0 and "blend_coverage_resolve" = 0 every k is 1.0f and nothing is resolved — every output and
 *   statistic equals the call with "blend_coverage" = 0, bit for bit; and where no pixel is usable (min_half_samples above every
 *   half's count) every T is 1: RTPBR_BUF_DENOISED_PIXELS holds rtpbr_denoise_coverage's bytes for the same parameters, the weight is
 *   1 and the depth K.
 *   rtpbr_get_counter name "blend_resolved": the pixels the resolve changed in the last such call (option 1, iterations > 0); 0
 *   before any; it blocks.  rtpbr_denoise_coverage's own count (its pixels_estimated) does not touch it.
 *   Errors: with the option at 1 and iterations > 0 the calls refuse what rtpbr_denoise_coverage refuses — RTPBR_EINVAL "coverage:
 *   grid x resolution out of range (1..65535)" when grid * width or grid * height exceeds 65535 — after their own parameter and
 *   state checks and before anything changes; otherwise they keep their own refusals and state rules.  rtpbr_set_option refuses
 *   a value out of range for each of the four keys in that key's own words.
 *   Memory: the coverage plane, its list and the two planes of rtpbr_denoise_coverage (k, 4 bytes; the linear colour, 12 bytes a
 *   pixel), shared with that call; no buffer id. */

/* ---- The level blend that fills pixels without samples (option "blend_fill"; counters "fill_filled", "fill_empty", "fill_deepest").
 *
 * In the three calls above a pixel whose count is 0 is no tap of any of the three ladders and is shown as rtpbr_post_process shows
 * it: a frame after rtpbr_reproject, or one traced on a lattice (rtpbr_select_mask + rtpbr_sample_selected), keeps its holes.  With
 * option "blend_fill" = 1 (rtpbr_set_option; 0 or 1, default 0) rtpbr_denoise_blend_levels, rtpbr_blend_error and
 * rtpbr_blend_error_display — and only they: every other call never reads the option and keeps its bytes, and the three calls never
 * read "denoise_fill" or "coverage_fill" — run the rule below.  It applies with K = iterations > 0; with iterations = 0 there is no
 * level to fill from, the option is not read, the holes stay and the three counters keep what they held.  With 0 everything above
 * holds, bit for bit.
 *   1. All three chains — image_buffer, half A, half B — run the filling level of rtpbr_denoise with option "denoise_fill" = 1 (see
 *      rtpbr_denoise): a pixel that holds no colour at a level (count 0 at level 1; not filled by an earlier level later) runs the
 *      same tap loop over the pixels of ITS object index that hold one, with the colour term of e taken as +0 (e = 0.0f; e = e +
 *      the normal term; e = e + the depth term), and holds the quotient s / sw from the next level on when sw > 0; otherwise it
 *      stays without a colour.  With option "blend_coverage" = 1 the chains run the filling level of rtpbr_denoise_coverage with
 *      option "coverage_fill" = 1 instead: every tap such a centre takes is weighted by k_q as well, on the one plane k.  A pixel that
 *      holds a colour runs its level exactly as without the option, and the pixels filled before are among its taps.  Each chain
 *      fills its own empty pixels: a pixel with samples in one half only (one sample: A = 1, B = 0) is filled in the other half's
 *      ladder.  F_0 .. F_K of a chain are its levels after remodulation, +0 where a level holds no colour.
 *   2. Pixels with samples (image_buffer[p].w > 0): everything above, on these ladders — the same usable test (cA >= m and cB >= m:
 *      a pixel whose count is 0 has cA + cB = 0 and m >= 1, so it is never usable and enters nobody's window sums), the same
 *      windows, t_k, T_k, depth, running colour, statistics, XA, XB, slope and error plane.
 *   3. A pixel whose count is 0, after the last level: if level K of image_buffer's chain holds a colour for it, it is shown with
 *      every t_k = 1 — RTPBR_BUF_DENOISED_PIXELS = the configured tone map of (F_K, 1), the remodulated last level by the pixel's own
 *      albedo, RTPBR_BUF_BLEND_WEIGHT holds 1 and RTPBR_BUF_BLEND_DEPTH holds K.  If it holds none (no pixel of its object with a colour within
 *      reach: 2 + 4 + .. + 2^K pixels along an axis) it is shown as rtpbr_post_process shows it, with weight 1 and depth 0.
 *   4. With "blend_coverage" = 1 the private linear plane L holds F_K for a filled pixel and +0 for one still empty, the last level
 *      writes beside it who has a colour (samples, or filled), and the resolve runs as rtpbr_denoise_coverage's with option
 *      "coverage_fill" = 1: the centre is resolved, and a neighbour serves in E2, exactly when it has a colour.  A filled pixel
 *      can be resolved and counts in "blend_resolved"; a pixel still empty shows what rtpbr_post_process shows.
 *   5. Every estimate and selection still sees a filled pixel as a pixel without samples: RTPBR_BUF_BLEND_ERROR holds 0 for it, its
 *      slope is 0, the statistics do not count it, and rtpbr_select_error / rtpbr_select_blend_error select it as they select a
 *      pixel without samples.  No error estimate of the filled colour is made.
 *   So: where image_buffer and both halves have no empty pixel, every output and statistic equals the call with "blend_fill" = 0,
 *   bit for bit; where no pixel is usable (min_half_samples above every half's count) RTPBR_BUF_DENOISED_PIXELS holds the bytes of
 *   rtpbr_denoise with "denoise_fill" = 1 (with "blend_coverage": of rtpbr_denoise_coverage with "coverage_fill" = 1) for the same
 *   parameters, and the three counters are that call's.
 *   rtpbr_get_counter names "fill_filled", "fill_empty", "fill_deepest" describe image_buffer's chain of the last filling call of ANY
 *   kind (this one, rtpbr_denoise with "denoise_fill" = 1, rtpbr_denoise_coverage with "coverage_fill" = 1; iterations > 0): the pixels
 *   without samples that hold a colour after level K, those that hold none, and the highest level, counted from 0, that filled one.
 *   The halves' chains are not counted.
 *   Errors: the calls keep their refusals and state rules.  rtpbr_set_option refuses a value other than 0 and 1 in the option's own
 *   words.  Memory: no buffer id; with "blend_coverage" the byte plane of rtpbr_denoise_coverage's filling form (1 byte a pixel). */

/* ---- Halves dealt per sample and carried through reprojection.
 *
 * Two switches of the section above, both off by default; with the defaults every buffer, counter and timing path is bit for bit
 * what it is without this call.  Every operation is f32, nothing fused.
 *
 * rtpbr_set_half_mode sets both; m == NULL restores the defaults.  The mode is plain context state: it survives rtpbr_refresh
 *   (which zeroes A and sh as before), rtpbr_set_config (a new resolution frees A and sh; the next dealing call makes them
 *   again), rtpbr_set_scene, rtpbr_reproject and rtpbr_reproject_scene.  Turning per_sample from 0 to 1 first does exactly what
 *   rtpbr_half_update does (same refusals: everything deposited so far is one batch, sh = image_buffer), then sets the mode;
 *   every other transition sets the mode, enqueues nothing and allocates nothing.  RTPBR_EINVAL for a NULL context or a field
 *   that is not 0 or 1.  A refused call changes nothing.
 *
 * per_sample = 1: rtpbr_sample(n) and rtpbr_sample_selected(n) of the complete-path form deal every staged sample to a half inside
 *   the pass that adds it to image_buffer.  For a pixel that receives samples, with b its image_buffer value, A its half and
 *   c = (r, g, b) each of its records in sample order:
 *     cB = b.w - A.w;                                                             (before the sample is added)
 *     if (A.w <= cB) { A.x = A.x + c.x; A.y = A.y + c.y; A.z = A.z + c.z; A.w = A.w + 1; }
 *     b.x += c.x; b.y += c.y; b.z += c.z; b.w += 1;                              (rtpbr_sample's own sum, unchanged)
 *   and after the pixel's last record of a sub-launch sh = b.  This is rtpbr_half_update's rule for a batch of one sample: samples
 *   alternate A, B, A, ... on a pixel whose halves are equal, and a pixel behind in one half catches up first; one rtpbr_sample(8)
 *   gives halves of 4 + 4.  The pass overwrites sh without reading it.  Pixels that receive no samples (unselected ones) keep A
 *   and sh bit for bit.  A dealing call allocates A and sh (zeroed) when they do not exist, is ordered behind asynchronous reads
 *   of RTPBR_BUF_HALF_BUFFER, and keeps item-linear staging whatever option stage_dense says (same bits, as
 *   rtpbr_sample_selected).  image_buffer, the work counters, sample_base, the timing and every other buffer are bit for bit those
 *   of the call without the mode, and the result does not depend on how the staging budget splits the call into sub-launches (it
 *   splits along samples).  An rtpbr_half_update after a dealing call finds d = 0 and changes nothing: the two may be mixed.  Noise
 *   tracking (rtpbr_set_noise_tracking) may be on at the same time: the moments' arithmetic and store order are untouched.
 *   While per_sample is on rtpbr_sample / rtpbr_sample_selected are refused with RTPBR_ESTATE, changing nothing, in the
 *   persistent-ray form (no per-sample records), with option precision = 1 (its unstaged instance keeps no records) and with
 *   tiles of world > 1.
 *
 * warp = 1: while A exists, rtpbr_reproject and rtpbr_reproject_scene carry half A with the image.  Before the gather A is copied
 *   into an internal history buffer (ordered behind asynchronous reads of RTPBR_BUF_HALF_BUFFER).  Per new pixel, over exactly
 *   the accepted taps q and weights w of the image (rtpbr_reproject), in tap order, with a_q the old A:
 *     SA = SA + w * a_q per component;        then A' = SA / Wt per component;
 *     when the cap applies (b.w > max_history before scaling): A' = A' * k per component, k = max_history / b.w the image's own;
 *     with no accepted tap A' = 0.
 *   sh becomes the warped image_buffer.  Because w >= 0, a_q.w <= b_q.w and every operation is monotone, 0 <= A'.w <= b'.w holds
 *   exactly: B' = b' - A' stays a valid half, and a pixel with history in both halves stays estimated across the move.
 *   image_buffer, RTPBR_BUF_MOTION, the moments and their snapshot and the features are bit for bit what they are without the
 *   mode.  With warp off, or before A exists, the calls do what the section above says (A is zeroed, sh becomes the warped
 *   image).  rtpbr_refresh and rtpbr_write_buffer(RTPBR_BUF_IMAGE_BUFFER) keep their rules in both modes. */
typedef struct rtpbr_half_mode {   /* 4-byte members, no padding */
    int32_t per_sample;   /* 0 (default) / 1: rtpbr_sample and rtpbr_sample_selected deal every sample to a half themselves */
    int32_t warp;         /* 0 (default) / 1: rtpbr_reproject and rtpbr_reproject_scene carry half A with the image          */
} rtpbr_half_mode;
/* Defaults (m == NULL): off.  raytracingpbr_amd.dataclass.HalfMode.DEFAULTS mirrors them (tests/test_half_mode_ref.py checks). */
#define RTPBR_HALF_MODE_DEFAULT_PER_SAMPLE 0
#define RTPBR_HALF_MODE_DEFAULT_WARP       0
int rtpbr_set_half_mode(rtpbr_ctx* ctx, const rtpbr_half_mode* m);   /* NULL = the defaults */

/* ---- The present stage: a display buffer becomes a packed 8-bit frame on the device, in one kernel.
 *
 * Every display buffer above is in the field layout — (W,H,3) f32, [x][y], y = 0 at the BOTTOM, y fastest — which no window,
 * encoder or image file takes: a host finishes the frame with a clamp, a quantisation and a transpose (what ti.tools.imwrite and
 * canvas.set_image do inside Taichi, src/main.py:55,64).  rtpbr_present does that step on the device and writes
 * RTPBR_BUF_PRESENT: (H,W,C) u8, row 0 = the TOP row of the picture, x fastest, C = 3 (RGB8) or 4 (RGBA8, alpha = 255): 3 or 4
 * bytes per pixel cross to the host instead of 12, and a consumer on the device takes the frame as it is.
 *
 * Every operation is f32, in this order, nothing fused.  Output element [r][x][c], r = 0 .. H-1 from the top:
 *   the field pixel is (x, y = H - 1 - r), buffer index x * H + y;
 *   v = channel c of the source there: RTPBR_PRESENT_PIXELS: image_pixels; RTPBR_PRESENT_DENOISED: denoised_pixels;
 *       RTPBR_PRESENT_ACCUM: tone_map(cfg, image_buffer[x * H + y]), the function rtpbr_post_process applies — what it WOULD write
 *       to image_pixels, bit for bit, without writing image_pixels, diff_buffer or diff_pixels;
 *   v = (v != v) ? 0 : v;   v = fminf(fmaxf(v, 0), 1);
 *   q = (uint8_t)(v * 255.0f + t)        (the product is rounded to f32 before the sum; the conversion truncates);
 *   dither = 0: t = 0.5f;
 *   dither = 1: t = (B[r & 7][x & 7] + 0.5f) * 0.015625f — the row is the TOP-DOWN row r, the column is x, the three channels of a
 *     pixel share t — with the 8 x 8 Bayer matrix
 *       B = {  0, 32,  8, 40,  2, 34, 10, 42,
 *             48, 16, 56, 24, 50, 18, 58, 26,
 *             12, 44,  4, 36, 14, 46,  6, 38,
 *             60, 28, 52, 20, 62, 30, 54, 22,
 *              3, 35, 11, 43,  1, 33,  9, 41,
 *             51, 19, 59, 27, 49, 17, 57, 25,
 *             15, 47,  7, 39, 13, 45,  5, 37,
 *             63, 31, 55, 23, 61, 29, 53, 21 };
 *     t runs over (k + 0.5) / 64, k = 0 .. 63: 0 < t < 1, so 0 stays 0 and 1 stays 255 in both modes, and the dithered value is at
 *     most one level from the undithered one.
 * With dither = 0 and source = RTPBR_PRESENT_PIXELS these are the bytes of the host path
 * (clip(nan_to_num(a, nan = 0), 0, 1) * 255 + 0.5 as uint8, then swapaxes(0, 1)[::-1]), byte for byte.
 *
 * The call is asynchronous on the context's stream and ordered behind an outstanding rtpbr_read_buffer_async of
 * RTPBR_BUF_PRESENT (that copy lands the previous frame).  It writes RTPBR_BUF_PRESENT and nothing else, leaves the work counters
 * alone, needs no flush of lazy shading (it reads image buffers only) and works with tiles of world > 1: it reads whole buffers,
 * as rtpbr_post_process does.  The buffer is allocated once, W * H * 4 bytes, by the first present; its size as
 * rtpbr_read_buffer / rtpbr_read_buffer_async / rtpbr_buffer_device_ptr report and require it is W * H * C of the LAST present.
 * rtpbr_write_buffer refuses it (RTPBR_EINVAL); rtpbr_set_config with a new resolution frees it.
 *
 * Errors: RTPBR_EINVAL for a NULL context or a field outside its range; RTPBR_ESTATE before rtpbr_set_config, and for
 * RTPBR_PRESENT_DENOISED before rtpbr_denoise / rtpbr_denoise_guided has made the buffer.  A refused call changes nothing. */
enum { RTPBR_PRESENT_PIXELS = 0,     /* RTPBR_BUF_IMAGE_PIXELS as it is                                         */
       RTPBR_PRESENT_DENOISED = 1,   /* RTPBR_BUF_DENOISED_PIXELS as it is                                      */
       RTPBR_PRESENT_ACCUM = 2 };    /* tone_map(cfg, image_buffer): rtpbr_post_process's colour, nothing written */
enum { RTPBR_PRESENT_RGB8 = 0,
       RTPBR_PRESENT_RGBA8 = 1 };    /* alpha = 255                                                             */
typedef struct rtpbr_present_params {   /* 4-byte members, no padding */
    int32_t source;        /* RTPBR_PRESENT_PIXELS / _DENOISED / _ACCUM     */
    int32_t format;        /* RTPBR_PRESENT_RGB8 / _RGBA8                   */
    int32_t dither;        /* 0: round to nearest; 1: ordered (Bayer 8 x 8) */
} rtpbr_present_params;
/* Defaults (p == NULL): image_pixels as RGBA8, no dither.  raytracingpbr_amd.dataclass.PresentParams.DEFAULTS mirrors them
 * (tests/test_present_ref.py checks). */
#define RTPBR_PRESENT_DEFAULT_SOURCE 0
#define RTPBR_PRESENT_DEFAULT_FORMAT 1
#define RTPBR_PRESENT_DEFAULT_DITHER 0
int rtpbr_present(rtpbr_ctx* ctx, const rtpbr_present_params* p);   /* NULL = the defaults */

/* ---- Coverage-aware denoise: sub-pixel coverage, purity-weighted taps, edge resolve.
 *
 * The features describe the ray through a pixel's CENTRE and rtpbr_denoise never takes a tap across object indices; a pixel's
 * samples, however, are jittered over the whole pixel.  On a silhouette the average in image_buffer is a mix of two objects, which
 * the filter takes for a pure member of the centre's object: the mix bleeds into every neighbour as a tap, and as a centre the
 * pixel is pulled to its own object's colour, which loses the anti-aliased edge.
 *
 * rtpbr_render_coverage writes the coverage plane and nothing else (it renders the features first when they are not valid).
 *   The plane: (W,H,4) i32 (n_own, second_object, n_second, n_sub) per pixel, in the field layout; it has no RTPBR_BUF_* id and
 *   is read with rtpbr_read_coverage.
 *   p == NULL: the defaults; only p->grid is used (power and resolve are checked as below): g = 2 or 4 sub-rays per axis,
 *   S = g * g.  RTPBR_EINVAL for another grid and where g * W or g * H exceeds 65535, the largest frame rtpbr_set_config
 *   accepts (sub-pixel coordinates stay far inside 32 bits: 4 * 65535 < 2^18).
 *   Whole frames only, with rtpbr_denoise's refusals.  Does not touch the work counters.
 *   Candidates: pixel p is a candidate when some pixel of its 3x3 neighbourhood inside the frame holds another index in
 *     RTPBR_BUF_FEAT_OBJECT.  Every other pixel gets (S, -2, 0, S) and is never marched.  LIMIT: a sliver of a foreign object that
 *     passes between the pixel centres of a neighbourhood makes no candidate and is missed.
 *   Sub-ray (a, b), a, b = 0 .. g-1, of candidate (px, py) is BY DEFINITION rtpbr_render_features' ray of pixel
 *     (g px + a, g py + b) of the configuration with width g W and height g H and everything else equal: same camera, march kind,
 *     shape data and frame uniform, no lens draws, no RNG draws.  Its object is the index it hits, -1 on a miss.
 *   n_own = the sub-rays whose object equals RTPBR_BUF_FEAT_OBJECT[p]; second_object = the most frequent other object among the
 *     sub-rays, ties to the smaller index (-1, the miss, is the smallest), -2 when there is none; n_second = its count; n_sub = S.
 *   Coverage is valid exactly as long as the features it was built from: whatever makes the features stale or renders them again
 *   (rtpbr_set_config / set_scene / set_camera / set_shape_data, rtpbr_render_features, the reprojections) makes the coverage
 *   stale, and the next call that needs it renders it again.  A stale plane keeps its bytes until then.
 *
 * rtpbr_denoise_coverage writes RTPBR_BUF_DENOISED_PIXELS (and the coverage plane when it is stale or of another grid) and nothing
 *   else.  p: rtpbr_denoise's parameters, defaults, refusals; v: NULL = the defaults below; RTPBR_EINVAL for power outside 0..8,
 *   resolve not 0 / 1, a bad grid.  It blocks when out != NULL (the statistics come back).  iterations = 0 is rtpbr_denoise's
 *   iterations = 0, byte for byte: no weight, no resolve.  Otherwise, with a_q = (float)n_own_q / (float)S:
 *   k_q = a_q * a_q * ... with `power` factors, multiplied left to right (power = 0: k_q = 1);
 *   the filter is rtpbr_denoise's with one change at every level: w = (h exp(-min(e, 80))) k_q for every tap but the centre's
 *     (dx = dy = 0: w = h exp(-min(e, 80)), as today); h, e, the skipped taps and the order of the sums as there.  F = its LINEAR
 *     result: the colour after remodulation, before the tone map.
 *   resolve = 1: for a pixel p with samples and n_second_p > 0, over the eight neighbours q = p + (dx, dy), dy = -1..1 (outer),
 *     dx = -1..1 (inner), inside the frame, with samples and RTPBR_BUF_FEAT_OBJECT[q] == second_object_p, sums from +0, no fma:
 *       w_q = k_q * (dx == 0 || dy == 0 ? 0.5f : 1.0f / 3.0f);  sw = sw + w_q;  s = s + w_q * F_q per channel;
 *     if sw > 0:  E2 = s / sw;  F_p <- ((float)n_own * F_p + (float)n_second * E2) / (float)(n_own + n_second) per channel,
 *     and the pixel counts as resolved.  The own side is F_p, the filter's result AT p (it carries the normal term: a lit face one
 *     pixel wide next to a dark one keeps its colour), never a mean of neighbours.
 *   denoised = the configured tone map of (F_p, 1); a pixel without samples shows what rtpbr_post_process shows, is nobody's tap
 *   and nobody's E2 neighbour, and is not resolved.  power = 0 with resolve = 0 gives rtpbr_denoise's bytes.
 *   out (may be NULL): pixels_estimated = the resolved pixels, pixels_above = the candidates, max_noise = the largest 1 - a.
 * Option "coverage_fill" (rtpbr_set_option; 0 or 1, default 0): with 0 everything above holds, bit for bit.  With 1,
 *   rtpbr_denoise_coverage — and only it: rtpbr_denoise, rtpbr_denoise_guided, rtpbr_denoise_error, the blend family,
 *   rtpbr_post_process, rtpbr_present and rtpbr_render_coverage never read the option and keep their bytes, and option "denoise_fill"
 *   still does not touch rtpbr_denoise_coverage — reconstructs the pixels without samples (the holes rtpbr_reproject* leaves, the
 *   pixels rtpbr_select_mask + rtpbr_sample_selected did not trace: both concentrate at silhouettes) inside the coverage-weighted
 *   levels, and resolves them as it resolves the others.  It applies with iterations > 0; iterations = 0 is the same call as with
 *   0, fills nothing, and the counters below keep the last filling call's values.
 *     A pixel is LIVE at level k when it has a colour on entry to that level: at level 0 the pixels with image_buffer[p].w > 0;
 *     the rest are EMPTY.  A tap q is skipped, for live and empty centres alike, when it is outside the frame, when it is not live
 *     on entry to this level, or when RTPBR_BUF_FEAT_OBJECT[q] != the centre's object index; an empty centre's object index is
 *     RTPBR_BUF_FEAT_OBJECT[p] (the features are rendered for every pixel).
 *     Live centre: the level above, operation for operation: w = (h exp(-min(e, 80))) k_q for every tap but its own.  The only
 *       difference is who is live — a pixel filled at an earlier level is a tap like any other.
 *     Empty centre p: the same loop, same tap order, with the colour term of e taken as +0,
 *       e = |n_p - n_q|^2 in + ((z_p - z_q) / max(z_p, 1e-6f))^2 iz (left to right), w = (h exp(-min(e, 80))) k_q for EVERY tap it
 *       takes (its own position is not live and is never a tap); sw = sw + w, s = s + w c_q per channel, from +0, no fma.
 *       If sw > 0 after the loop, c_p = s / sw: p is live from the next level on and counts as FILLED AT LEVEL k.  Otherwise p
 *       stays empty.  Every level reads only its input: a fill never sees another fill of the same level.
 *     Filling is decided by the COMPUTED sum, sw > 0 — it is not purely a rule about reach as rtpbr_denoise's fill is: k_q is 0
 *       where n_own_q = 0 (power >= 1), and at power 8 the product of a small k_q with a weight near h exp(-80) ~ 7e-38 can
 *       underflow to 0 in f32 (a denormal product is kept and counts as > 0).  A pixel all of whose reachable
 *       live taps weigh 0 stays empty at that level.  Only at power = 0 (k_q = 1) does the rule reduce to "some tap of the level is
 *       live on the pixel's object".
 *     Demodulation: at level 0 a tap's colour is its average divided by max(albedo_p, 1e-3f), the centre's own albedo (one
 *       constant per object); at the last level a filled pixel is remodulated by its own albedo, as every pixel is.  That linear
 *       colour is its F_p.
 *     Resolve: "with samples" above reads "has a colour after the last level", for the centre p and for its eight E2 neighbours
 *       alike: a filled pixel with n_second > 0 is resolved by the same formula and counts in pixels_estimated.
 *     A pixel still empty after the last level shows what rtpbr_post_process shows, is nobody's tap and nobody's E2 neighbour,
 *       and is not resolved.
 *   So: on a frame where every pixel has samples both settings give the same bytes and statistics at every iterations; with
 *   resolve = 0 and iterations = 1 every pixel that has samples carries the bytes it has with the option off; power = 0 with
 *   resolve = 0 gives the bytes and the counters of rtpbr_denoise with option denoise_fill = 1.  image_buffer, the features, the
 *   coverage plane's contents, the selection, the work counters and sample_base are untouched; the refusals are those above.
 *   rtpbr_get_counter names "fill_filled", "fill_empty" and "fill_deepest" (defined at rtpbr_denoise) describe the last filling call
 *   of ANY kind: rtpbr_denoise with denoise_fill = 1, rtpbr_denoise_coverage with coverage_fill = 1 or a level blend call with
 *   blend_fill = 1 (image_buffer's chain), iterations > 0.
 *   Keeps one more (W,H) 1-byte plane (who has a colour after the last level: written by that level, read by the resolve; no
 *   buffer id), made by the first such call and freed by rtpbr_set_config with a new resolution. */
typedef struct rtpbr_coverage_params {   /* 4-byte members, no padding */
    int32_t grid;       /* sub-rays per axis: 2 or 4                                                     */
    int32_t power;      /* 0..8: a tap's weight is (n_own / S)^power                                     */
    int32_t resolve;    /* 1: mix the second object's 3x3 mean into the pixels that hold two objects     */
} rtpbr_coverage_params;
/* Defaults (NULL).  The power is the one with the best worst-case whole-frame RMSE ratio to rtpbr_denoise over Cornell v3 at 4 and
 * 64 spp and the src/ Tokyo scene (tools/coverage_sweep.py).
 * raytracingpbr_amd.dataclass.CoverageParams.DEFAULTS mirrors them (tests/test_coverage_ref.py checks). */
#define RTPBR_COVERAGE_DEFAULT_GRID    4
#define RTPBR_COVERAGE_DEFAULT_POWER   4
#define RTPBR_COVERAGE_DEFAULT_RESOLVE 1
int rtpbr_render_coverage(rtpbr_ctx* ctx, const rtpbr_coverage_params* p);
int rtpbr_denoise_coverage(rtpbr_ctx* ctx, const rtpbr_denoise_params* p, const rtpbr_coverage_params* v, rtpbr_noise_stats* out);
/* Copy the coverage plane to host memory (blocking), as the last coverage call wrote it: nbytes = W * H * 16.  RTPBR_ESTATE before
 * the first coverage call and after rtpbr_set_config with a new resolution (the plane is freed with the feature buffers);
 * RTPBR_EINVAL for another size. */
int rtpbr_read_coverage(rtpbr_ctx* ctx, void* dst, size_t nbytes);

/* Block until everything enqueued on the context has finished (its stream, and the copies of rtpbr_read_buffer_async). */
int rtpbr_sync(rtpbr_ctx* ctx);

/* field.to_numpy() / from_numpy(): copy a whole buffer to/from host memory (blocking). */
int rtpbr_read_buffer(rtpbr_ctx* ctx, int which, void* dst, size_t nbytes);
int rtpbr_write_buffer(rtpbr_ctx* ctx, int which, const void* src, size_t nbytes);

/* Page-locked host memory for the destination of rtpbr_read_buffer(): a host that shows every frame (src/main.py:62-64 hands
 * image_pixels to the window once per render()) reads into the SAME buffer again and again, and a page-locked one takes the copy
 * at the link's rate without the driver's staging.  Plain memory works as before; this is an optimisation the caller opts into.
 * Freed by rtpbr_host_free() or with the context. */
int rtpbr_host_alloc(rtpbr_ctx* ctx, size_t nbytes, void** ptr);
int rtpbr_host_free(rtpbr_ctx* ctx, void* ptr);

/* Handing a frame over WITHOUT stalling the device (round 6).  The reference's window takes image_pixels on the device
 * (`canvas.set_image(image_pixels)`, src/main.py:64: the frame never visits the host) and its loop goes straight on to the
 * next render(); rtpbr_read_buffer() above is the blocking `field.to_numpy()`.  Two more ways out:
 *
 * rtpbr_buffer_device_ptr: the DEVICE address and size of a buffer — zero copy for a consumer on the same GPU (display
 *   interop, a video encoder, a torch tensor through __cuda_array_interface__).  The consumer orders itself behind the
 *   context's work with rtpbr_get_stream() (or calls rtpbr_sync()); the address stays valid until rtpbr_set_config()
 *   changes the resolution or the context is destroyed, and the next rtpbr_post_process() / rtpbr_sample() overwrites
 *   the contents, as the reference's next render() does.
 *
 * rtpbr_read_buffer_async: enqueue the copy of a buffer into PAGE-LOCKED host memory (a block of rtpbr_host_alloc; EINVAL
 *   otherwise — a pageable destination would make the copy synchronous) behind everything enqueued on the context so
 *   far, on a copy stream of its own, and return a ticket at once.  The context's later work does NOT wait for the copy —
 *   frame k's read-back overlaps frame k+1's sample kernels — except the first call that would overwrite the buffer
 *   being read (the next rtpbr_post_process() for image_pixels): that one is ordered behind the copy on the device, the
 *   host still does not block.  rtpbr_read_wait(ticket) blocks the HOST until that copy has landed in `dst`.  Up to 8
 *   reads may be outstanding; taking a 9th ticket first waits for the oldest. */
int rtpbr_buffer_device_ptr(rtpbr_ctx* ctx, int which, void** device_ptr, size_t* nbytes);
int rtpbr_read_buffer_async(rtpbr_ctx* ctx, int which, void* dst, size_t nbytes, int* ticket);
int rtpbr_read_wait(rtpbr_ctx* ctx, int ticket);

/* Multi-GPU gather support.  pack: copy this rank's tiles of image_buffer, tile-major,
 * into a DEVICE buffer of rtpbr_packed_bytes() bytes (all ranks get the same padded size
 * so one RCCL gather moves them).  unpack: scatter a packed buffer that belongs to rank
 * `src_rank` into this context's image_buffer.  Both run on the context's stream. */
int rtpbr_packed_bytes(rtpbr_ctx* ctx, size_t* nbytes);
int rtpbr_pack_tiles(rtpbr_ctx* ctx, void* device_dst);
int rtpbr_unpack_tiles(rtpbr_ctx* ctx, const void* device_src, int src_rank);

/* ---- the ONE collective of the multi-GPU path, on RCCL directly (rt_rccl.hip).
 * Replaces nothing in the reference (it is single-device); completes rtpbr_set_tiles / pack / unpack
 * so that hosts without PyTorch can render on N GPUs: every rank packs its tiles, one ncclGather (rccl.h:745) moves
 * them to rank 0, rank 0 scatters them into its full image_buffer (T7) — all enqueued on the context's stream.
 * One process per GPU: rank 0 obtains a 128-byte id, ships it to the other ranks by the host's own means, every rank
 * calls rtpbr_rccl_init (collective, like ncclCommInitRank, rccl.h:220), then rtpbr_gather_tiles (collective).
 * One process driving G contexts: rtpbr_rccl_init_all (ncclCommInitAll, rccl.h:236) and rtpbr_gather_tiles_all.
 * rank/world must equal the ones given to rtpbr_set_tiles.  librccl is dlopen-ed at the first of these calls. */
int rtpbr_rccl_unique_id(void* out, size_t nbytes);                       /* nbytes >= 128 */
int rtpbr_rccl_init(rtpbr_ctx* ctx, const void* unique_id, size_t nbytes, int rank, int world);
int rtpbr_rccl_init_all(rtpbr_ctx** ctxs, int n);
int rtpbr_gather_tiles(rtpbr_ctx* ctx);
int rtpbr_gather_tiles_all(rtpbr_ctx** ctxs, int n);
/* What RCCL itself reports for this context's communicator: ncclCommCount (rccl.h:378), ncclCommUserRank (:400) and the
 * library's version (ncclGetVersion, :164) — so that a caller can show that the collective really spans `world` ranks. */
int rtpbr_rccl_info(rtpbr_ctx* ctx, int* nranks, int* rank, int* version);

/* Measurement hooks (SURVEY.md §5 tracing row, §8(d)). */
int rtpbr_get_counters(rtpbr_ctx* ctx, rtpbr_counters* out);         /* blocking */
/* One counter by name: the six above, plus "mlp_wave_evals" / "mlp_lane_evals" — 32-ray half passes of the
 * wave-cooperative neural-SDF network (bunny_sdf_glass.py:149-203 on the matrix cores) and the ray evaluations they
 * were needed for; their ratio / 32 is the slot utilisation of the MLP; "fill_filled" / "fill_empty" / "fill_deepest": the last
 * rtpbr_denoise with option denoise_fill = 1, rtpbr_denoise_coverage with option coverage_fill = 1 (see rtpbr_denoise) or level
 * blend call with option blend_fill = 1 (image_buffer's chain; see rtpbr_blend_error_display);
 * "blend_resolved": the pixels the resolve changed in the last rtpbr_denoise_blend_levels / rtpbr_blend_error /
 * rtpbr_blend_error_display with option blend_coverage = 1 (see rtpbr_blend_error_display).  EINVAL for an unknown name. */
int rtpbr_get_counter(rtpbr_ctx* ctx, const char* name, unsigned long long* out);
/* Device time (HIP events on the context's stream) of the trace kernel launches and of
 * all kernels of the last rtpbr_sample() call, in milliseconds (blocking).  Option "timing" = 0 records no events
 * (every event is a few microseconds of idle queue between two small kernels: 8 us of a 160 us one-step launch) —
 * these two calls then return RTPBR_ESTATE. */
int rtpbr_last_sample_ms(rtpbr_ctx* ctx, float* trace_ms, float* total_ms, int* launches);
/* Device time of the primary_rays launches of the last rtpbr_sample() call (0 launches when
 * the primary raycasts ran inside the trace kernel: option "primary_split" 0, neural SDF). */
int rtpbr_last_primary_ms(rtpbr_ctx* ctx, float* primary_ms, int* launches);
/* Raw stream handle (hipStream_t) so callers can order their own work after ours. */
int rtpbr_get_stream(rtpbr_ctx* ctx, void** stream);
/* Tuning knobs that do not change results.  Keys: "staging_bytes" (sub-launch staging budget),
 * "scheduler" (-1 auto, 0 in-register refill / lock-step, 1 per-wave LDS ray pool),
 * "wait_lanes" (scheduler 0), "shade_lanes", "swap_lanes" (0 = automatic, the default: 8 in the complete-path pool kernel, 12 in the
 * persistent-ray one), "refill_lanes", "ready_low" (scheduler 1), "waves_per_cu",
 * "residency" (persistent-ray form, pool scheduler: bounce-steps a pixel stays resident in a wave that owns more pixels
 * than the 128 it can hold; a power of two, default 32), "grid_blocks" (same kernel: workgroups to launch, 0 = automatic),
 * "cover_blocks" (the sub-ray kernel of rtpbr_render_coverage: workgroups to launch, 0 = automatic),
 * "denoise_fill" (this one changes a result, rtpbr_denoise's alone: 1 = pixels without samples are reconstructed from their
 * neighbours, 0 = default; see rtpbr_denoise), "coverage_fill" (the same for rtpbr_denoise_coverage, and its result alone: 1 = pixels
 * without samples are reconstructed inside the coverage-weighted levels and resolved, 0 = default; see rtpbr_denoise_coverage),
 * "blend_coverage" (changes the results of rtpbr_denoise_blend_levels, rtpbr_blend_error and rtpbr_blend_error_display alone: 1 = their
 * ladders are the coverage-weighted filter's and two-object pixels are resolved, 0 = default) with "blend_coverage_grid" (2 or 4,
 * default 4), "blend_coverage_power" (0..8, default 4) and "blend_coverage_resolve" (0 or 1, default 1), the rtpbr_coverage_params of
 * those calls; see rtpbr_blend_error_display, "blend_fill" (changes the results of the same three calls alone: 1 = their ladders fill
 * the pixels without samples and the frame shows them, 0 = default),
 * "drain_lanes" (complete-path pool kernel: once the work has run out and nothing is parked, a wave with at most this many marching
 * lanes finishes their raycasts in the culled wave march of the primary kernel; default 16, 0 = never),
 * "primary_lean" (1, default: the coherent primary-ray kernel marches on in a one-object loop while its whole wave needs one object),
 * "src_chain" (persistent-ray form, fused launches: 1, default = when the plan finds the launch as long as its heaviest pixel's
 * dependency chain AND the device has room beside the pool kernel's grid, the heaviest pixels — the chain set — run in the chain
 * kernel on a second stream, alone or in small groups per wave; 0 = never, 2 = whenever the plan says so), "chain_waves" (the most
 * waves the chain set may take, default 1024; the pool kernel's grid makes room for them), "chain_np_max" (frames of more local
 * pixels than this are throughput-bound and get no chain set, default 2 500 000),
 * "src_split" (persistent-ray form: a launch of at most this many bounce-steps runs as a wavefront split — per step one
 * coherent kernel for roulette / deposit / camera ray, one for the raycasts on the cost-ordered pixel list, one for shading —
 * instead of the fused pool kernel; 0 = never, default 1), "split_wait" (its march kernel refills lanes when this many are
 * free, default 24),
 * "src_op" (round 6: bit 0 = while at most 8 lanes of a wave march — the tail of a one-step launch, a chain wave of a few pixels —
 * the wave evaluates nearest() OBJECT-PARALLEL: lane (r, j) evaluates object j for the r-th marching ray from the LDS table and a DPP
 * butterfly over each group of eight lanes returns nearest / second / third, bit-identical; split march and chain kernels; bit 1 =
 * the fused pool kernel too, only in builds with -DRT_POOL_OP=1: it spills there; bit 2 = the per-lane lean loop: when every marching
 * lane holds a valid bound but for a DIFFERENT object, each lane evaluates its own object from the LDS table in one loop; default 7),
 * "split_head" (split march kernel: the
 * cost-ordered list's heavy head interleaved over the groups, one entry per group, instead of filling the first groups: -1 = for
 * frames of at most 600 000 pixels (default), 0 never, 1 always),
 * "src_lazy" (one-step launches of the persistent-ray form, i.e. the wavefront split; 1, default: a launch leaves its shading to the
 * next launch's gen pass — one pass over ray_buffer instead of two, one kernel less per launch — and every call that could see the
 * difference launches it first: readers and writers of ray_buffer (rtpbr_buffer_device_ptr of ray_buffer ends the lazy mode for the
 * context), rtpbr_get_counter(s), every setter, rtpbr_refresh, a launch of another kind; rtpbr_post_process and reads of the image
 * buffers do not need it.  0: every launch shades.  Same bits either way),
 * "env_packed" (1, default: an environment uploaded as 8-bit texels is read as RGBA8 texels + the 256-entry table of
 * (c / 255 * exposure)^gamma — the same floats, a quarter of the bytes, same speed; 0 = float4 texels),
 * "src_track" (same kernel: 1 = tracked-object march steps — a lane that knows a lower bound of every object but the
 * nearest one evaluates only that one, exactly; heavy waves always use them), "sparse_lanes" (... other waves while at
 * most this many lanes march, 0 = never; default 24), "leave_x8" (cost of a shading pass in eighths of a march iteration:
 * the march loop is left when the lane-iterations wasted by finished lanes and parked contexts reach it; default 24),
 * "src_plan" (1: the pool kernel records every pixel's march steps and re-orders its ownership by them — heaviest pixels
 * first, the very heaviest in waves of their own), "plan_interval" (bounce-steps on record before a re-plan, default 64),
 * "heavy_mean_x16" / "heavy_bulk_x16" (a pixel is heavy when its cost exceeds both that many sixteenths of the mean pixel
 * and of a wave's share of the frame in march iterations; defaults 48, 8), "heavy_own" (pixels per heavy wave, <= 128,
 * default 80), "tiny_own" / "tiny_waves" (the very heaviest pixels: waves of at most tiny_own pixels, tiny_waves of them —
 * a quarter of the grid when the launch is as long as its longest chain), "heavy_prio" (heavy waves raise their issue
 * priority), "age_tune" (1, default: the light waves' shares are weighted by the residency slot of their block — the k-th
 * block of a CU is the k-th oldest wave of its SIMD and the issue arbiter favours the older wave — with weights the library
 * tunes from the lifetimes it measures, so that the waves of a SIMD end together; 0 = equal shares), "age_weights" (fixed
 * weights instead, one hex digit per slot, oldest first),
 * "primary_split" (primary raycasts in their own coherent lock-step kernel with wave-level
 * object culling; pool scheduler, analytic shapes: 0 never, 1 for launches of >= 2^23 samples
 * (default), 2 always), "specialize" (1: use the instance compiled
 * for the scene's rotation signature when there is one), "lazy_sqrt" (1: all-box scenes pick the
 * nearest box on squared distances and take one exact square root per march step),
 * "mlp_mfma", "mlp_lanes" (neural SDF: run the network when this many lanes wait for it), "mlp_full" (compute both
 * 32-slot halves of a pass when at least this many wait, else the first 32 by rank),
 * "jit" (per-scene kernels compiled at run time by hipcc --genco from the sources next to the library — what Taichi's
 * JIT does for the reference: object loop unrolled, each object's shape function and rotation class fixed at compile
 * time, src/scene.py:44-56 — cached under $RTPBR_JIT_CACHE / ~/.cache/rtpbr: -1 (default) when no ahead-of-time
 * specialisation serves the scene, 0 never, 1 always but falling back to the ahead-of-time kernels if compilation is
 * impossible, 2 always and an error otherwise), "jit_bake" (1: the run-time instance also carries the scene's object
 * table and the whole rtpbr_config except seed and frame as compile-time constants — one code object per scene and
 * configuration; for offline renders of a fixed scene),
 * "jit_waves" (waves per SIMD the run-time pool kernel is compiled for; 0 = as the ahead-of-time instances),
 * "chunk" (work items a wave claims per atomic, at most 8192; 0 = automatic: total / (waves x 64) clamped to [256, 1024]),
 * "timing" (1, the default: rtpbr_sample() brackets its kernels with HIP events for rtpbr_last_sample_ms /
 * rtpbr_last_primary_ms; 0: none),
 * "stage_dense" (complete-path pool kernel, run-time instances only — the code is compiled in on request; 1: a wave appends the finished samples of a claim to the claim's own
 * stretch of the staging in completion order, with one byte that says which sample each is, and the accumulate kernel puts them
 * back in sample order — the claim is then the largest size <= 256 that is a whole multiple or a whole fraction of the launch's
 * samples per pixel, and a launch that has none (or a "chunk" that is none) keeps the item-linear records; 0, the default:
 * item-linear records always.  Same bits either way; 21 % fewer HBM writes and 7 % more time on the 1080p x 256 spp step),
 * "reserve_spp" (allocate the staging of a call of that many samples per pixel now instead of on
 * first use), "select_lattice" (build the selection of a lattice on the device now: the adaptive-sampling section),
 * "sample_base" (absolute index of the next sample: checkpoint/resume).
 * Returns RTPBR_EINVAL for unknown keys or out-of-range values. */
int rtpbr_set_option(rtpbr_ctx* ctx, const char* key, long long value);

/* Ahead-of-time compilation of the scene-specialised kernels (round 6) — NO DEVICE NEEDED.  Taichi compiles the reference's
 * kernels at first call on the machine that runs them (ti.init, src/config.py:5; ti.static unrolling, src/scene.py:44-56);
 * option "jit" does the same here and needs hipcc + the kernel sources on the target.  rtpbr_jit_prebuild compiles, on a BUILD
 * machine, exactly the code object rtpbr_sample() would ask for with this scene (objects, scale10), configuration, camera, tile
 * partition (tile_w, tile_h, world; rank does not matter) and options ("key=value key=value ...", as rtpbr_set_option:
 * jit, jit_bake, precision, mlp_mfma, ...) into $RTPBR_JIT_CACHE and returns its path.  Code objects placed in the catalog
 * directory next to the library (raytracingpbr_amd/data/jit, or $RTPBR_JIT_CATALOG) are found by rtpbr_sample() BEFORE it
 * forks a compiler: a target without hipcc runs the baked kernels of the scenes it ships with.  `python -m
 * raytracingpbr_amd.prebuild` fills the catalog for the BASELINE scenes (called by the package's build step). */
int rtpbr_jit_prebuild(const rtpbr_object* objects, int n, int scale10, const rtpbr_config* cfg, const rtpbr_camera* cam,
                       int tile_w, int tile_h, int world, const char* options, char* path_out, size_t path_cap);

#ifdef __cplusplus
}
#endif
#endif /* RTPBR_H */
