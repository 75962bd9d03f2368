// rt_capi.hip — host side of the C ABI declared in include/rtpbr.h.
//
// One rtpbr_ctx owns one HIP stream and every device buffer of one renderer instance (what
// the Taichi runtime owns in the reference: src/fileds.py:7-15, src/scene.py:38-41,
// src/ibl.py:16-17).  Each entry point replaces one Taichi kernel launch or field access of
// the reference; see the header for the line-by-line mapping.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "rt_ctx.hpp"
#include "rt_launch_plan.hpp"
#include "rt_coverage.hpp"
#include "rt_features.hpp"
#include "rt_reproject.hpp"
#include "rt_noise.hpp"
#include "rt_half.hpp"
#include "rt_present.hpp"
#include "rt_select.hpp"

using namespace rt;

static void derive_launch(rtpbr_ctx* c, RtJitKey* key, bool* want, bool* strict_error);
static int half_restart(rtpbr_ctx* c, bool snapshot_image, bool keep_a = false);
static int noise_stats_read(rtpbr_ctx* c, rtpbr_noise_stats* out);
extern "C" int rtpbr_set_option(rtpbr_ctx* c, const char* key, long long value);
extern "C" int rtpbr_set_tiles(rtpbr_ctx* c, int tw, int th, int rank, int world);
extern "C" int rtpbr_set_camera(rtpbr_ctx* c, const rtpbr_camera* cam);

static thread_local char g_err[512];
int rt_fail(int code, const char* fmt, const char* a) {
    snprintf(g_err, sizeof g_err, fmt, a);
    return code;
}
int rt_fail_hip(const char* expr, hipError_t e) {
    snprintf(g_err, sizeof g_err, "%s failed: %s", expr, hipGetErrorString(e));
    return RTPBR_EHIP;
}
static int fail(int code, const char* fmt, const char* a = "") { return rt_fail(code, fmt, a); }
#define HIP_TRY(expr) RT_HIP_TRY(expr)

static int set_dev(rtpbr_ctx* c) {
    if (c->headless) return RTPBR_OK;       // (a context without a device: rtpbr_jit_prebuild derives launch constants on the host only)
    HIP_TRY(hipSetDevice(c->device));
    return RTPBR_OK;
}

// The lazy shading of the split's one-step launches (rt_ctx.hpp src_lazy): launch what the last such launch left for the next one's gen
// pass.  Called by everything that could tell the difference.
static int flush_shade(rtpbr_ctx* c) {
    if (!c->shade_pending) return RTPBR_OK;
    c->shade_pending = false;
    if (int r = set_dev(c)) return r;
    rtpbr_ctx::Params& P = c->P;
    const uint32_t keep = P.sample_base;
    P.sample_base = c->shade_pending_base;
    int rc = RTPBR_OK;
    if (c->jit_mod) rc = rt_jit_launch(c->jit_mod->src_shade, P, (unsigned)(((long long)P.np + 255) / 256), c->stream);
    else launch_src_shade(P, c->kind, c->stream);
    P.sample_base = keep;
    return rc;
}

extern "C" const char* rtpbr_last_error(void) { return g_err; }
extern "C" const char* rtpbr_backend(void) { return "hip-gfx950"; }

extern "C" int rtpbr_destroy(rtpbr_ctx* c);
static int create_resources(rtpbr_ctx* c) {
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    HIP_TRY(hipMalloc(&c->objfull, sizeof(ObjFull) * MAX_OBJ));
    HIP_TRY(hipMalloc(&c->team_counter, 1024 * 64));
    // the work counters of a launch and the claim counters of the complete-path kernels in one allocation: ONE fill per rtpbr_sample()
    // (a fill is a dispatch of its own: ~15 us between two small launches)
    constexpr size_t counters_bytes = (sizeof(Counters) + 64 + 255) / 256 * 256;
    HIP_TRY(hipMalloc(&c->counters_buf[0], 2 * counters_bytes));
    c->counters_buf[1] = reinterpret_cast<Counters*>(reinterpret_cast<char*>(c->counters_buf[0]) + counters_bytes);
    HIP_TRY(hipMemsetAsync(c->counters_buf[0], 0, 2 * counters_bytes, c->stream));
    c->counters_clean[0] = c->counters_clean[1] = true;
    c->counters = c->counters_buf[0];
    c->work_counter = reinterpret_cast<unsigned int*>(reinterpret_cast<char*>(c->counters) + sizeof(Counters));
    // timing events carry no data to the host (a read-back synchronises the stream itself): without the system-scope fence an event
    // costs the queue less (rocprofv3: ~10 us of idle queue per default event between two small kernels)
    HIP_TRY(hipEventCreateWithFlags(&c->ev_total1, hipEventDisableSystemFence));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, c->device));
    c->n_cu = prop.multiProcessorCount;
    return RTPBR_OK;
}

extern "C" int rtpbr_create(int device, rtpbr_ctx** out) {
    if (!out) return fail(RTPBR_EINVAL, "out is NULL");
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return fail(RTPBR_EINVAL, "no such HIP device");
    rtpbr_ctx* c = new rtpbr_ctx();
    c->device = device;
    const int r = create_resources(c);
    if (r != RTPBR_OK) {            // g_err already says which call failed; release whatever was created
        rtpbr_destroy(c);
        return r;
    }
    *out = c;
    return RTPBR_OK;
}

// ---- the frame buffers (RT_FRAME_BUFFERS, rt_ctx.hpp): every allocation, free and public lookup of a row is one of these three
// the rows' names for frame_need
enum FrameRow {
#define X(m, T, bytes, group, zeroed, id, writable) ROW_##m,
    RT_FRAME_BUFFERS(X)
#undef X
};

// Allocate the rows that do not exist yet, zero-filled on the stream where the row says so.  The caller has made every refusal
// of its own: a refused call allocates nothing.
static int frame_need(rtpbr_ctx* c, std::initializer_list<FrameRow> rows) {
    const size_t np = (size_t)c->cfg.width * c->cfg.height;
    constexpr bool reported = false;
    for (const FrameRow row : rows) {
        switch (row) {
#define X(m, T, bytes, group, zeroed, id, writable)                                                       \
    case ROW_##m:                                                                                         \
        if (!c->m) {                                                                                      \
            if (const hipError_t e = hipMalloc(&c->m, bytes)) return rt_fail_hip("hipMalloc(" #m ")", e); \
            if (zeroed) HIP_TRY(hipMemsetAsync(c->m, 0, bytes, c->stream));                               \
        }                                                                                                 \
        break;
            RT_FRAME_BUFFERS(X)
#undef X
        }
    }
    return RTPBR_OK;
}

// Free and null every row of `groups` (FRAME_*), with the state that describes the group's contents
static void frame_free(rtpbr_ctx* c, unsigned groups) {
#define X(m, T, bytes, group, zeroed, id, writable) \
    if (groups & (group)) {                         \
        (void)hipFree(c->m);                        \
        c->m = nullptr;                             \
    }
    RT_FRAME_BUFFERS(X)
#undef X
    if (groups & FRAME_FEATURES) c->feat_valid = c->cov_valid = false;
    if (groups & FRAME_SELECTION) {
        c->sel_count = 0;
        c->have_selection = false;
        c->sel_tiers = 1;
        for (uint32_t& l : c->sel_cum) l = 0;
        c->sel_blocks_tiered = false;
    }
    if (groups & FRAME_PRESENT) c->present_channels = 0;
}

extern "C" int rtpbr_destroy(rtpbr_ctx* c) {
    if (!c) return RTPBR_OK;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);      // (an asynchronous read-back may still be copying out of the buffers)
    frame_free(c, FRAME_ALL);
    (void)hipFree(c->objfull);
    (void)hipFree(c->env);
    (void)hipFree(c->env8);
    (void)hipFree(c->env_lut);
    (void)hipFree(c->bunny);
    (void)hipFree(c->stage);
    (void)hipFree(c->primary);
    (void)hipFree(c->cost_buffer);
    (void)hipFree(c->march_out);
    (void)hipFree(c->noise_stats);
    (void)hipFree(c->fill_counts);
    (void)hipFree(c->blend_resolved);
    (void)hipFree(c->order);
    (void)hipFree(c->plan);
    rt_rccl_release(c);
    rt_jit_release(c->jit_mod);
    c->jit_mod = nullptr;
    (void)hipFree(c->team_counter);
    for (void* hb : c->host_blocks) (void)hipHostFree(hb);
    c->host_blocks.clear();
    c->host_sizes.clear();
    (void)hipFree(c->counters_buf[0]);
    for (hipEvent_t e : c->ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->evp) (void)hipEventDestroy(e);
    if (c->ev_total1) (void)hipEventDestroy(c->ev_total1);
    if (c->stream2) {
        (void)hipStreamSynchronize(c->stream2);
        (void)hipStreamDestroy(c->stream2);
    }
    if (c->copy_stream) {
        (void)hipStreamSynchronize(c->copy_stream);
        (void)hipStreamDestroy(c->copy_stream);
    }
    if (c->ev_read_ready) (void)hipEventDestroy(c->ev_read_ready);
    for (hipEvent_t e : c->ev_read_done)
        if (e) (void)hipEventDestroy(e);
    if (c->plan_rb_host) (void)hipHostFree(c->plan_rb_host);
    if (c->ev_plan_rb) (void)hipEventDestroy(c->ev_plan_rb);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return RTPBR_OK;
}

static void update_tiles(rtpbr_ctx* c) {
    Params& P = c->P;
    const int W = c->cfg.width, H = c->cfg.height;
    int tw = c->tile_w, th = c->tile_h;
    if (c->world <= 1 || tw <= 0 || th <= 0) {
        if (tw <= 0 || th <= 0) {
            tw = W;
            th = H;
        }
    }
    P.tile_w = tw;
    P.tile_h = th;
    P.ntx = (W + tw - 1) / tw;
    P.nty = (H + th - 1) / th;
    P.rank = c->rank;
    P.world = c->world;
    int ntiles = P.ntx * P.nty;
    P.n_local_tiles = (ntiles + c->world - 1) / c->world;
    P.np = P.n_local_tiles * tw * th;
    // the src/ pool kernel's cost-ordered ownership lists LOCAL pixels: a new partition starts without a plan
    c->order_valid = false;
    c->cost_steps = 0;
    c->plan_np = 0;
}

// Work items (padded local pixels x samples per launch) are 32-bit: a rank's padded pixel count must
// leave room for at least one sample per launch plus the chunks the last waves claim past the end.
static int check_local_pixels(int W, int H, int tw, int th, int world) {
    if (world <= 1 || tw <= 0 || th <= 0) { tw = W; th = H; world = world < 1 ? 1 : world; }
    const long long ntx = (W + tw - 1) / tw, nty = (H + th - 1) / th;
    const long long local = (ntx * nty + world - 1) / world;
    if (local * tw * th > (1LL << 30)) return fail(RTPBR_EINVAL, "more than 2^30 (padded) pixels per rank: use more ranks or smaller frames");
    return RTPBR_OK;
}

extern "C" int rtpbr_set_config(rtpbr_ctx* c, const rtpbr_config* cfg) {
    if (!c || !cfg) return fail(RTPBR_EINVAL, "null argument");
    if (cfg->width <= 0 || cfg->height <= 0 || cfg->width > 65535 || cfg->height > 65535)
        return fail(RTPBR_EINVAL, "resolution out of range (1..65535)");
    if (cfg->max_raymarch <= 0 || cfg->max_raytrace <= 0) return fail(RTPBR_EINVAL, "max_raymarch/max_raytrace must be > 0");
    if (int r = check_local_pixels(cfg->width, cfg->height, c->tile_w, c->tile_h, c->world)) return r;
    if (int r = set_dev(c)) return r;
    if (int r = flush_shade(c)) return r;
    bool realloc_buf = (!c->have_cfg || c->cfg.width != cfg->width || c->cfg.height != cfg->height) && !c->headless;
    c->cfg = *cfg;
    c->P.cfg = *cfg;
    c->have_cfg = true;
    c->feat_valid = false;
    c->history_ok = false;
    if (realloc_buf) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (c->copy_stream) HIP_TRY(hipStreamSynchronize(c->copy_stream));
        for (int& t : c->read_pending) t = -1;
        frame_free(c, FRAME_ALL);
        if (int r = frame_need(c, {ROW_image_buffer, ROW_image_pixels, ROW_ray_buffer, ROW_diff_buffer, ROW_diff_pixels})) return r;
    }
    // bunny animation uniform: t = pi*frame/120 (bunny_sdf_glass.py:214)
    float t = PI * (float)cfg->frame / 120.0f;
    sincos_(t, &c->P.anim_s, &c->P.anim_c);
    c->P.anim_bz = cfg->anim_bob * c->P.anim_s;
    update_tiles(c);
    return RTPBR_OK;
}

// Euler -> matrix, src/util.py:36-42: M = Rz @ Ry @ Rx (row major)
static void m3_mul(const float* a, const float* b, float* o) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            o[i * 3 + j] = a[i * 3 + 0] * b[0 * 3 + j] + a[i * 3 + 1] * b[1 * 3 + j] + a[i * 3 + 2] * b[2 * 3 + j];
}
static void rotate(const float* rad, float* m) {
    float sx = (float)sin((double)rad[0]), cx = (float)cos((double)rad[0]);
    float sy = (float)sin((double)rad[1]), cy = (float)cos((double)rad[1]);
    float sz = (float)sin((double)rad[2]), cz = (float)cos((double)rad[2]);
    float rz[9] = {cz, sz, 0, -sz, cz, 0, 0, 0, 1};
    float ry[9] = {cy, 0, -sy, 0, 1, 0, sy, 0, cy};
    float rx[9] = {1, 0, 0, 0, cx, sx, 0, -sx, cx};
    float t[9];
    m3_mul(rz, ry, t);
    m3_mul(t, rx, m);
}

// exact sparsity pattern of a world->local matrix (see to_local): 0 entries must be +-0, the axis entry 1.0f
static int rotation_class(const float* m) {
    auto z = [&](int i) { return m[i] == 0.0f; };
    auto one = [&](int i) { return m[i] == 1.0f; };
    for (int i = 0; i < 9; i++)
        if (!std::isfinite(m[i])) return ROT_GENERAL;
    if (one(0) && one(4) && one(8) && z(1) && z(2) && z(3) && z(5) && z(6) && z(7)) return ROT_IDENT;
    if (one(0) && z(1) && z(2) && z(3) && z(6)) return ROT_X;
    if (one(4) && z(1) && z(3) && z(5) && z(7)) return ROT_Y;
    if (one(8) && z(2) && z(5) && z(6) && z(7)) return ROT_Z;
    return ROT_GENERAL;
}

// First listed signature (RT_BOX_SIGNATURES) whose every specialised class fits the object's matrix;
// an identity matrix fits every single-axis class.  0 = the general instance.
static uint32_t choose_signature(const ObjM* objm) {
    int cls[8];
    for (int i = 0; i < 8; i++) cls[i] = rotation_class(objm[i].m);
    const uint32_t sigs[] = {
#define RT_SIG_ITEM(sig, ...) sig,
        RT_BOX_SIGNATURES(RT_SIG_ITEM, 0)
#undef RT_SIG_ITEM
    };
    for (uint32_t sig : sigs) {
        bool ok = true;
        for (int i = 0; i < 8 && ok; i++) {
            const int want = sig_cls(sig, i);
            ok = want == ROT_GENERAL || want == cls[i] || cls[i] == ROT_IDENT;
        }
        if (ok) return sig;
    }
    return 0;
}

// Fill a march table: the general 64-byte blocks, or the signature's packed layout (rt_types.hpp:
// only the dwords each object's rotation class reads, wide-load friendly).
static void pack_table(const ObjM* src, int n, uint32_t sig, ObjM* dst_table) {
    memset(dst_table, 0, sizeof(ObjM) * MAX_OBJ);
    if (sig == 0) {
        memcpy(dst_table, src, sizeof(ObjM) * (size_t)n);
        return;
    }
    float* f = reinterpret_cast<float*>(dst_table);
    for (int i = 0; i < n; i++) {
        const ObjM& o = src[i];
        const int cls = sig_cls(sig, i);
        float* d = f + sig_offset(sig, i);
        if (cls == ROT_GENERAL) {
            memcpy(d, &o, sizeof o);
            continue;
        }
        d[0] = o.px, d[1] = o.py, d[2] = o.pz;
        if (cls == ROT_IDENT) {
            d[3] = o.sx, d[4] = o.sy, d[5] = o.sz;
            continue;
        }
        const int e[3][4] = {{4, 5, 7, 8}, {0, 2, 6, 8}, {0, 1, 3, 4}};   // X, Y, Z: the four entries that are not 0 / 1
        for (int k = 0; k < 4; k++) d[3 + k] = o.m[e[cls - ROT_X][k]];
        d[7] = o.sx, d[8] = o.sy, d[9] = o.sz;
    }
}

// An object as rtpbr_set_scene stores it: position and scale times ten if asked, the world->local matrix from `rotation`
static rtpbr_object stored_object(const rtpbr_object& in, int scale10) {
    rtpbr_object o = in;
    rtpbr_transform& t = o.transform;
    if (scale10)
        for (int k = 0; k < 3; k++) {
            t.position[k] *= 10.0f;
            t.scale[k] *= 10.0f;
        }
    float rad[3] = {t.rotation[0] * DEG2RAD, t.rotation[1] * DEG2RAD, t.rotation[2] * DEG2RAD};
    rotate(rad, t.matrix);
    return o;
}

extern "C" int rtpbr_set_scene(rtpbr_ctx* c, const rtpbr_object* objs, int n, int scale10) {
    if (!c || !objs) return fail(RTPBR_EINVAL, "null argument");
    if (n <= 0 || n > MAX_OBJ) return fail(RTPBR_EINVAL, "object count must be 1..32");
    for (int i = 0; i < n; i++)   // validate before touching the context
        if (objs[i].type < RTPBR_SHAPE_NONE || objs[i].type > RTPBR_SHAPE_BUNNY) return fail(RTPBR_EINVAL, "unknown shape type");
    if (int r = set_dev(c)) return r;
    if (int r = flush_shade(c)) return r;
    c->feat_valid = false;
    c->history_ok = false;
    ObjFull full[MAX_OBJ];
    memset(full, 0, sizeof full);
    bool all_box = true, all_bunny = true, any_bunny = false;
    for (int i = 0; i < n; i++) {
        c->obj[i] = stored_object(objs[i], scale10);
        const rtpbr_transform& t = c->obj[i].transform;
        ObjM& m = c->objm[i];
        m.px = t.position[0]; m.py = t.position[1]; m.pz = t.position[2];
        memcpy(m.m, t.matrix, sizeof m.m);
        m.sx = t.scale[0]; m.sy = t.scale[1]; m.sz = t.scale[2];
        m.type = c->obj[i].type;
        ObjFull& f = full[i];
        memcpy(&f, &m, sizeof m);
        const rtpbr_material& mt = c->obj[i].material;
        memcpy(f.albedo, mt.albedo, 12);
        memcpy(f.emission, mt.emission, 12);
        f.roughness = mt.roughness; f.metallic = mt.metallic; f.transmission = mt.transmission; f.ior = mt.ior;
        if (m.type != RTPBR_SHAPE_BOX) all_box = false;
        if (m.type != RTPBR_SHAPE_BUNNY) all_bunny = false;
        else any_bunny = true;
    }
    c->scene_sig = (all_box && n == 8) ? choose_signature(c->objm) : 0;
    c->n_obj = n;
    c->P.n_obj = n;
    c->kind = all_box ? KIND_BOXES : (all_bunny && n == 1) ? KIND_BUNNY : any_bunny ? KIND_MIXED : KIND_GENERIC;
    if (!c->headless) {
        HIP_TRY(hipMemcpyAsync(c->objfull, full, sizeof(ObjFull) * n, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));  // `full` is a stack buffer
    }
    c->have_scene = true;
    return RTPBR_OK;
}

// Test hook, HOST ONLY (no device needed): the signature an 8-box scene would be rendered with and
// its packed march table (128 floats), for tests/test_host_logic.py.
extern "C" int rtpbr_test_signature(const rtpbr_object* objs, int n, int scale10, uint32_t* sig, float* table) {
    if (!objs || !sig || n != 8) return RTPBR_EINVAL;
    ObjM objm[MAX_OBJ];
    memset(objm, 0, sizeof objm);
    bool all_box = true;
    for (int i = 0; i < n; i++) {
        rtpbr_transform t = objs[i].transform;
        if (scale10)
            for (int k = 0; k < 3; k++) {
                t.position[k] *= 10.0f;
                t.scale[k] *= 10.0f;
            }
        float rad[3] = {t.rotation[0] * DEG2RAD, t.rotation[1] * DEG2RAD, t.rotation[2] * DEG2RAD};
        rotate(rad, t.matrix);
        ObjM& m = objm[i];
        m.px = t.position[0]; m.py = t.position[1]; m.pz = t.position[2];
        memcpy(m.m, t.matrix, sizeof m.m);
        m.sx = t.scale[0]; m.sy = t.scale[1]; m.sz = t.scale[2];
        m.type = objs[i].type;
        if (m.type != RTPBR_SHAPE_BOX) all_box = false;
    }
    *sig = all_box ? choose_signature(objm) : 0;
    if (table) {
        ObjM packed[MAX_OBJ];
        pack_table(objm, n, *sig, packed);
        memcpy(table, packed, 128 * sizeof(float));
    }
    return RTPBR_OK;
}

// The key of the run-time instance of a scene (rt_jit.hip): everything the generated code depends on.  P carries the
// launch constants that get baked (box thresholds, tile geometry, scheduler thresholds, culling decision).
static void box_thresholds(float rho, int lazy_sqrt, Params& P) {
    P.box_lazy = (lazy_sqrt && rho >= 0.0f && rho <= 1e15f) ? 1 : 0;
    // the squared-distance keys of nearest_boxes_lazy are carried scaled by 4 (exact): thresholds likewise
    P.box_four_rho = 4.0f * rho;
    P.box_rho2m = (float)((double)rho * (double)rho * (1.0 + 1.0 / 524288.0));
    if (P.box_rho2m > 0.0f) P.box_rho2m = nextafterf(P.box_rho2m, INFINITY);
    P.box_4rho2m = nextafterf((float)(4.0 * (double)rho * (double)rho * (1.0 + 1.0 / 524288.0)), INFINITY);
    P.box_rho2m *= 4.0f;
    P.box_4rho2m *= 4.0f;
}
static RtJitKey make_jit_key(int kind, int n_obj, const ObjM* objm, const rtpbr_config& cfg, const Params& P, bool persistent, int jit_bake,
                             int jit_waves, bool jit_bunny, int fast = 0) {
    RtJitKey key{};
    key.fast = fast;
    key.kind = kind;
    key.n_obj = n_obj;
    for (int i = 0; i < n_obj; i++) {
        key.types |= (unsigned long long)(objm[i].type + 1) << (4 * i);
        key.sig |= (unsigned)rotation_class(objm[i].m) << (3 * i);
    }
    key.cull = P.cull_ok;
    key.form = persistent ? 1 : 0;
    if (jit_bunny) key.sig = 0;
    key.waves = kind == KIND_BOXES ? 6 : kind == KIND_BUNNY ? 4 : 5;      // as the ahead-of-time instances (RT_POOL_WAVES*)
    if (jit_waves > 0) key.waves = jit_waves;
    key.baked = jit_bake;
    key.table = reinterpret_cast<const unsigned*>(objm);
    if (key.baked) {
        rtpbr_config b = cfg;
        b.seed = 0;
        b.frame = 0;
        memcpy(key.cfg_words, &b, sizeof b);
        key.extra[0] = (unsigned)P.box_lazy;
        memcpy(&key.extra[1], &P.box_four_rho, 4);
        memcpy(&key.extra[2], &P.box_rho2m, 4);
        memcpy(&key.extra[3], &P.box_4rho2m, 4);
        const int ints[8] = {P.tile_w, P.tile_h, P.ntx, P.nty, P.world, P.shade_lanes, P.swap_lanes, P.mlp_mfma};
        memcpy(key.ints, ints, sizeof ints);
        if (key.baked == 2) memcpy(key.cam_words, &P.cam, sizeof key.cam_words);
    }
    return key;
}

// Test / tooling hook, HOST ONLY (no device needed): compile the BAKED run-time instance of a scene + configuration the
// way rtpbr_sample() would (single rank, default scheduler thresholds) and return the code object's path, so that the
// generated ISA can be inspected in a container without a GPU (tools/jit_offline.py).
extern "C" int rtpbr_test_jit_build_baked(const rtpbr_object* objs, int n, int scale10, const rtpbr_config* cfg, int waves, int fast, char* path_out, size_t cap) {
    if (!objs || !cfg || n <= 0 || n > 8) return fail(RTPBR_EINVAL, "bad arguments");
    ObjM objm[MAX_OBJ];
    memset(objm, 0, sizeof objm);
    bool all_box = true;
    for (int i = 0; i < n; i++) {
        rtpbr_transform t = objs[i].transform;
        if (scale10)
            for (int k = 0; k < 3; k++) {
                t.position[k] *= 10.0f;
                t.scale[k] *= 10.0f;
            }
        float rad[3] = {t.rotation[0] * DEG2RAD, t.rotation[1] * DEG2RAD, t.rotation[2] * DEG2RAD};
        rotate(rad, t.matrix);
        ObjM& m = objm[i];
        m.px = t.position[0]; m.py = t.position[1]; m.pz = t.position[2];
        memcpy(m.m, t.matrix, sizeof m.m);
        m.sx = t.scale[0]; m.sy = t.scale[1]; m.sz = t.scale[2];
        m.type = objs[i].type;
        if (m.type != RTPBR_SHAPE_BOX) all_box = false;
        if (m.type == RTPBR_SHAPE_BUNNY) return fail(RTPBR_EINVAL, "analytic shapes only");
    }
    rtpbr_ctx defaults;
    Params P{};
    P.cfg = *cfg;
    P.cull_ok = 1;
    P.tile_w = cfg->width, P.tile_h = cfg->height, P.ntx = 1, P.nty = 1, P.world = 1;
    P.shade_lanes = defaults.shade_lanes, P.swap_lanes = cfg->kernel_form == RTPBR_FORM_PERSISTENT_RAY ? 12 : 8;
    box_thresholds(cfg->box_round, 1, P);
    const RtJitKey key = make_jit_key(all_box ? KIND_BOXES : KIND_GENERIC, n, objm, *cfg, P, cfg->kernel_form == RTPBR_FORM_PERSISTENT_RAY, 1, waves, false, fast);
    std::string p;
    if (int r = rt_jit_build(key, &p, nullptr)) return r;
    if (path_out && cap) snprintf(path_out, cap, "%s", p.c_str());
    return RTPBR_OK;
}

// Ahead-of-time compilation of the run-time instance of ONE scene + configuration (+ camera, tiles, options) — NO DEVICE NEEDED:
// a headless context takes the same set_config / set_scene / set_camera / set_tiles / set_option calls a rendering host makes,
// derive_launch() forms the key rtpbr_sample() would ask for, and rt_jit_build() compiles it into $RTPBR_JIT_CACHE (or finds it
// there / in the catalog shipped next to the library, raytracingpbr_amd/data/jit).  __graft_entry__.build() fills that catalog for the
// BASELINE scenes this way, so that a target without hipcc still runs the scene-specialised kernels (rt_jit.hip looks there
// before it forks a compiler).  `options`: "key=value key=value ..." as for rtpbr_set_option (jit, jit_bake, precision, ...).
extern "C" int rtpbr_jit_prebuild(const rtpbr_object* objs, int n, int scale10, const rtpbr_config* cfg, const rtpbr_camera* cam,
                                  int tile_w, int tile_h, int world, const char* options, char* path_out, size_t cap) {
    if (!objs || !cfg || !cam) return fail(RTPBR_EINVAL, "rtpbr_jit_prebuild: scene, configuration and camera are required");
    rtpbr_ctx ctx;
    rtpbr_ctx* c = &ctx;
    c->headless = true;
    if (world > 1)
        if (int r = rtpbr_set_tiles(c, tile_w, tile_h, 0, world)) return r;
    if (int r = rtpbr_set_config(c, cfg)) return r;
    if (int r = rtpbr_set_scene(c, objs, n, scale10)) return r;
    if (int r = rtpbr_set_camera(c, cam)) return r;
    std::string opt = options ? options : "";
    for (size_t i = 0; i < opt.size();) {
        while (i < opt.size() && opt[i] == ' ') i++;
        size_t j = opt.find(' ', i);
        if (j == std::string::npos) j = opt.size();
        if (j > i) {
            const std::string kv = opt.substr(i, j - i);
            const size_t e = kv.find('=');
            if (e == std::string::npos) return fail(RTPBR_EINVAL, "rtpbr_jit_prebuild: options are key=value pairs (%s)", kv.c_str());
            if (int r = rtpbr_set_option(c, kv.substr(0, e).c_str(), atoll(kv.c_str() + e + 1))) return r;
        }
        i = j;
    }
    RtJitKey key{};
    bool want = false, strict_error = false;
    derive_launch(c, &key, &want, &strict_error);
    if (!want) return fail(RTPBR_ESTATE, "rtpbr_jit_prebuild: with these options rtpbr_sample() would not use a run-time instance for this scene "
                                         "(option jit, <= 8 analytic shapes or the neural shape with jit_bake, pool scheduler)");
    std::string p;
    if (int r = rt_jit_build(key, &p, nullptr)) return r;
    if (path_out && cap) snprintf(path_out, cap, "%s", p.c_str());
    return RTPBR_OK;
}

extern "C" int rtpbr_get_scene(rtpbr_ctx* c, rtpbr_object* objs, int n) {
    if (!c || !objs || n < 0 || n > c->n_obj) return fail(RTPBR_EINVAL, "bad get_scene arguments");
    memcpy(objs, c->obj, (size_t)n * sizeof *objs);
    return RTPBR_OK;
}

// thin-lens frame, src/camera.py:11-31 (same operation order as the oracle's camera_frame)
extern "C" int rtpbr_set_camera(rtpbr_ctx* c, const rtpbr_camera* cam) {
    if (!c || !cam) return fail(RTPBR_EINVAL, "null argument");
    if (int r = flush_shade(c)) return r;
    c->feat_valid = false;
    c->cam = *cam;
    vec3 lf = mk(cam->lookfrom[0], cam->lookfrom[1], cam->lookfrom[2]);
    vec3 la = mk(cam->lookat[0], cam->lookat[1], cam->lookat[2]);
    vec3 up = mk(cam->vup[0], cam->vup[1], cam->vup[2]);
    float theta = cam->vfov * DEG2RAD;
    float hh = tanf(theta * 0.5f);
    float hw = cam->aspect * hh;
    vec3 z = normalize(lf - la);
    vec3 x = normalize(cross(up, z));
    vec3 y = cross(z, x);
    vec3 hwfx = x * (hw * cam->focus);
    vec3 hhfy = y * (hh * cam->focus);
    vec3 llc = ((lf - hwfx) - hhfy) - z * cam->focus;
    vec3 hor = hwfx * 2.0f, ver = hhfy * 2.0f;
    CamFrame& f = c->P.cam;
    f.lf[0] = lf.x; f.lf[1] = lf.y; f.lf[2] = lf.z;
    f.x[0] = x.x; f.x[1] = x.y; f.x[2] = x.z;
    f.y[0] = y.x; f.y[1] = y.y; f.y[2] = y.z;
    f.llc[0] = llc.x; f.llc[1] = llc.y; f.llc[2] = llc.z;
    f.hor[0] = hor.x; f.hor[1] = hor.y; f.hor[2] = hor.z;
    f.ver[0] = ver.x; f.ver[1] = ver.y; f.ver[2] = ver.z;
    f.lens_radius = cam->aperture * 0.5f;
    c->have_cam = true;
    return RTPBR_OK;
}

// Image(path) + Image.process(exposure, gamma): src/ibl.py:14-23, postprocessor.adjust :17-21
extern "C" int rtpbr_set_env(rtpbr_ctx* c, const void* texels, int w, int h, int fmt, float exposure, float gamma) {
    if (!c || !texels) return fail(RTPBR_EINVAL, "null argument");
    if (w <= 0 || h <= 0) return fail(RTPBR_EINVAL, "bad env size");
    if (fmt != RTPBR_ENV_RGB8 && fmt != RTPBR_ENV_RGB32F) return fail(RTPBR_EINVAL, "bad env format");
    if (int r = set_dev(c)) return r;
    if (int r = flush_shade(c)) return r;
    c->history_ok = false;
    size_t n = (size_t)w * h;
    std::vector<float4> host(n);
    if (fmt == RTPBR_ENV_RGB8) {
        const uint8_t* s = (const uint8_t*)texels;
        float lut[256];
        for (int i = 0; i < 256; i++) lut[i] = pow_(((float)i / 255.0f) * exposure, gamma);
        for (size_t i = 0; i < n; i++) host[i] = make_float4(lut[s[i * 3]], lut[s[i * 3 + 1]], lut[s[i * 3 + 2]], 0.0f);
    } else {
        const float* s = (const float*)texels;
        for (size_t i = 0; i < n; i++) host[i] = make_float4(s[i * 3], s[i * 3 + 1], s[i * 3 + 2], 0.0f);
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    (void)hipFree(c->env);
    (void)hipFree(c->env8);
    (void)hipFree(c->env_lut);
    c->env = nullptr;
    c->env8 = nullptr;
    c->env_lut = nullptr;
    HIP_TRY(hipMalloc(&c->env, n * sizeof(float4)));
    HIP_TRY(hipMemcpy(c->env, host.data(), n * sizeof(float4), hipMemcpyHostToDevice));
    if (fmt == RTPBR_ENV_RGB8) {
        // ... and as the reference's image really is (T9): 8-bit texels + the table Image.process() amounts to
        const uint8_t* s8 = (const uint8_t*)texels;
        std::vector<uint32_t> packed(n);
        for (size_t i = 0; i < n; i++) packed[i] = (uint32_t)s8[i * 3] | ((uint32_t)s8[i * 3 + 1] << 8) | ((uint32_t)s8[i * 3 + 2] << 16);
        float lut[256];
        for (int i = 0; i < 256; i++) lut[i] = pow_(((float)i / 255.0f) * exposure, gamma);
        HIP_TRY(hipMalloc(&c->env8, n * sizeof(uint32_t)));
        HIP_TRY(hipMalloc(&c->env_lut, sizeof lut));
        HIP_TRY(hipMemcpy(c->env8, packed.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c->env_lut, lut, sizeof lut, hipMemcpyHostToDevice));
    }
    c->P.env = c->env;
    c->P.env_w = w;
    c->P.env_h = h;
    return RTPBR_OK;
}

extern "C" int rtpbr_set_shape_data(rtpbr_ctx* c, int shape, const float* data, int n) {
    if (!c || !data) return fail(RTPBR_EINVAL, "null argument");
    if (shape != RTPBR_SHAPE_BUNNY || n != 625) return fail(RTPBR_EINVAL, "only the bunny MLP (625 weights) takes shape data");
    if (int r = set_dev(c)) return r;
    if (int r = flush_shade(c)) return r;
    // device layout: the hidden layers' matrices in chain order (rt_device.hpp): [k][i][m][j] <- caller's [k][m][i][j]
    float dev[625];
    memcpy(dev, data, sizeof dev);
    for (int layer = 0; layer < 2; layer++)
        for (int k = 0; k < 4; k++)
            for (int m = 0; m < 4; m++)
                for (int i = 0; i < 4; i++)
                    for (int j = 0; j < 4; j++)
                        dev[64 + layer * 272 + k * 68 + i * 16 + m * 4 + j] = data[64 + layer * 272 + k * 68 + m * 16 + i * 4 + j];
    c->feat_valid = false;
    c->history_ok = false;
    if (!c->bunny) HIP_TRY(hipMalloc(&c->bunny, 625 * sizeof(float)));
    HIP_TRY(hipMemcpy(c->bunny, dev, 625 * sizeof(float), hipMemcpyHostToDevice));
    c->P.bunny = c->bunny;
    return RTPBR_OK;
}

extern "C" int rtpbr_set_tiles(rtpbr_ctx* c, int tw, int th, int rank, int world) {
    if (!c) return fail(RTPBR_EINVAL, "null ctx");
    if (world < 1 || rank < 0 || rank >= world) return fail(RTPBR_EINVAL, "bad rank/world");
    if (world > 1 && (tw <= 0 || th <= 0)) return fail(RTPBR_EINVAL, "tile size must be > 0 when world > 1");
    if (int r = flush_shade(c)) return r;
    c->tile_w = tw;
    c->tile_h = th;
    c->rank = rank;
    c->world = world;
    if (c->have_cfg) {
        if (int r = check_local_pixels(c->cfg.width, c->cfg.height, tw, th, world)) return r;
        update_tiles(c);
    }
    return RTPBR_OK;
}

// A call that WRITES the buffers of `mask` (bit RTPBR_BUF_*) on the context's stream is ordered behind an asynchronous
// read-back that still copies out of them (rtpbr_read_buffer_async) — on the device: the host does not block.
int rt_order_after_reads(rtpbr_ctx* c, unsigned mask) {
    for (int b = 0; b < RT_PUBLIC_BUFFERS; b++)
        if (((mask >> b) & 1u) && c->read_pending[b] >= 0) {
            // (a copy that has landed already needs no ordering: a cross-stream wait is a barrier packet the command processor
            // resolves in ~20 us — per frame that is what separates a pipelined viewer from the device-only rate — a query is ~1 us)
            const hipError_t q = hipEventQuery(c->ev_read_done[c->read_pending[b] & 7]);
            if (q == hipErrorNotReady) {
                (void)hipGetLastError();
                HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_read_done[c->read_pending[b] & 7], 0));
            } else if (q != hipSuccess) {
                return rt_fail_hip("hipEventQuery(read-back)", q);
            }
            c->read_pending[b] = -1;
        }
    return RTPBR_OK;
}
// ... the masks the writers pass
enum : unsigned {
    W_IMAGE_BUFFER = 1u << RTPBR_BUF_IMAGE_BUFFER,
    W_IMAGE_PIXELS = 1u << RTPBR_BUF_IMAGE_PIXELS,
    W_RAY_BUFFER = 1u << RTPBR_BUF_RAY_BUFFER,
    W_DIFF_BUFFER = 1u << RTPBR_BUF_DIFF_BUFFER,
    W_DIFF_PIXELS = 1u << RTPBR_BUF_DIFF_PIXELS,
    W_FEATURES = (1u << RTPBR_BUF_FEAT_ALBEDO) | (1u << RTPBR_BUF_FEAT_NORMAL) | (1u << RTPBR_BUF_FEAT_DEPTH) | (1u << RTPBR_BUF_FEAT_OBJECT),
    W_DENOISED = 1u << RTPBR_BUF_DENOISED_PIXELS,
    W_MOTION = 1u << RTPBR_BUF_MOTION,
    W_MOMENTS = 1u << RTPBR_BUF_MOMENTS,
    W_NOISE = 1u << RTPBR_BUF_NOISE,
    W_SELECTION = 1u << RTPBR_BUF_SELECTION,
    W_PRESENT = 1u << RTPBR_BUF_PRESENT,
    W_HALF = 1u << RTPBR_BUF_HALF_BUFFER,
    W_ERROR = 1u << RTPBR_BUF_DENOISED_ERROR,
    W_BLEND = 1u << RTPBR_BUF_BLEND_WEIGHT,
    W_DEPTH = 1u << RTPBR_BUF_BLEND_DEPTH,
    W_BLEND_ERROR = 1u << RTPBR_BUF_BLEND_ERROR,
};

extern "C" int rtpbr_refresh(rtpbr_ctx* c) {
    if (!c || !c->have_cfg) return fail(RTPBR_ESTATE, "set_config first");
    if (int r = set_dev(c)) return r;
    if (int r = flush_shade(c)) return r;
    if (int r = rt_order_after_reads(c, W_IMAGE_BUFFER | W_RAY_BUFFER | W_DIFF_BUFFER | W_DIFF_PIXELS | (c->noise_moments ? W_MOMENTS : 0u))) return r;
    size_t n = (size_t)c->cfg.width * c->cfg.height;
    if (c->noise_moments) {      // the noise estimate starts over with the image
        HIP_TRY(hipMemsetAsync(c->noise_moments, 0, n * sizeof(float4), c->stream));
        HIP_TRY(hipMemsetAsync(c->noise_snapshot, 0, n * sizeof(float4), c->stream));
    }
    if (int r = half_restart(c, false)) return r;      // the halves start over with the image
    launch_refresh(c->image_buffer, c->ray_buffer, c->diff_buffer, c->diff_pixels, c->cfg.adaptive_sampling, n, c->stream);
    HIP_TRY(hipGetLastError());
    c->history_ok = true;
    return RTPBR_OK;
}

static void pack_objects(rtpbr_ctx* c, Params& P) { pack_table(c->objm, c->n_obj, P.box_sig, P.objm); }

// Staging and, for the primary split, the primary records (what an item takes of each: rt_launch_plan.hpp).
// Grown on demand; hipMalloc of several GB takes 50..700 ms, so callers that time whole frames can
// reserve up front (option "reserve_spp").
// Returns RTPBR_ENOMEM (nothing allocated, no sticky HIP error) when the device has no room: the caller then renders
// with fewer samples per launch instead of failing.
// staging of `items` samples: the 12-byte records, then (dense staging) one fill count per chunk of >= 32 items and one byte per record
static size_t stage_bytes(size_t items) { return items * sizeof(StageRec) + (items / DENSE_CHUNK_MIN + 2) * sizeof(uint32_t) + items; }
static int staging_alloc(rtpbr_ctx* c, void** ptr, size_t* cap, size_t need) {
    if (need <= *cap) return RTPBR_OK;
    HIP_TRY(hipStreamSynchronize(c->stream));
    (void)hipFree(*ptr);
    *ptr = nullptr;
    *cap = 0;
    const hipError_t e = hipMalloc(ptr, need);
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        *ptr = nullptr;
        return RTPBR_ENOMEM;
    }
    if (e != hipSuccess) return rt_fail_hip("hipMalloc(staging)", e);
    *cap = need;
    return RTPBR_OK;
}
static int ensure_staging(rtpbr_ctx* c, size_t items, bool split, bool stage = true) {
    if (stage)
        if (int r = staging_alloc(c, (void**)&c->stage, &c->stage_cap, stage_bytes(items))) return r;
    if (split)
        if (int r = staging_alloc(c, (void**)&c->primary, &c->primary_cap, items * PRIMARY_REC_BYTES)) return r;
    return RTPBR_OK;
}

// next event of a reusable pool; a failed hipEventCreate is reported, never recorded
static int next_event_of(std::vector<hipEvent_t>& pool, int& used, hipEvent_t* out) {
    if (used == (int)pool.size()) {
        hipEvent_t e = nullptr;
        HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableSystemFence));      // (timing only: see create_resources)
        pool.push_back(e);
    }
    *out = pool[used++];
    return RTPBR_OK;
}
#define NEXT_EVENT(pool, used, var)                                   \
    hipEvent_t var = nullptr;                                         \
    if (int r_ = next_event_of(pool, used, &var)) return r_

static int trace_grid(rtpbr_ctx* c, uint32_t total_items, bool selected = false) {
    const int per_cu = selected ? trace_selected_blocks_per_cu(c->kind, c->n_obj, c->P.scheduler)
                 : c->jit_mod ? c->jit_mod->trace_blocks_per_cu
                              : trace_blocks_per_cu(c->kind, c->n_obj, c->P.box_sig, c->scheduler < 0 ? 1 : c->scheduler);
    return (int)capped_grid(blocks_per_cu(per_cu, c->waves_per_cu), c->n_cu, total_items);
}

// Everything of a launch that is decided on the HOST from the context's state (configuration, scene, camera, tiles, options) and
// that the run-time instance's key depends on: shared by rtpbr_sample() and rtpbr_jit_prebuild() (which has no device), so that
// a code object compiled ahead of time for a catalog scene IS the one rtpbr_sample() will ask for.  *want = a run-time instance
// is to be used (key filled); *strict_error = option jit = 2 and no instance exists for this scene.
static void derive_launch(rtpbr_ctx* c, RtJitKey* key, bool* want, bool* strict_error) {
    Params& P = c->P;
    P.cfg = c->cfg;
    P.cam.inv_w = 1.0f / (float)c->cfg.width;
    P.cam.inv_h = 1.0f / (float)c->cfg.height;
    P.image_buffer = c->image_buffer;
    P.image_pixels = c->image_pixels;
    P.ray_buffer = c->ray_buffer;
    P.diff_buffer = c->diff_buffer;
    P.diff_pixels = c->diff_pixels;
    P.objfull = c->objfull;
    P.env8 = (c->env_packed && c->env8) ? c->env8 : nullptr;
    P.env_lut = c->env_lut;
    P.work_counter = c->work_counter;
    P.counters = c->counters;
    P.wait_lanes = c->wait_lanes;
    P.shade_lanes = c->shade_lanes;
    P.refill_lanes = c->refill_lanes;
    P.ready_low = c->ready_low;
    // lanes that must have finished before the march loop is left for a swap: the src/ form's swap moves 15-word contexts and
    // runs once per ~8 raycasts — 12 instead of 8 is +1.5 % at every frame size (profiles/r04); the complete-path kernel stays at 8
    P.swap_lanes = c->swap_lanes > 0 ? c->swap_lanes : (c->cfg.kernel_form == RTPBR_FORM_PERSISTENT_RAY ? 12 : 8);
    P.sparse_lanes = c->sparse_lanes;
    P.mlp_lanes = c->mlp_lanes;
    P.mlp_full = c->mlp_full;
    P.mlp_mfma = c->mlp_mfma;
    P.scheduler = c->scheduler < 0 ? 1 : c->scheduler;
    // the pool kernel's parked records hold the bounce number in 11 bits
    if (c->cfg.kernel_form == RTPBR_FORM_COMPLETE_PATH && c->cfg.max_raytrace > 2047) P.scheduler = 0;
    // signature instances exist for the complete-path kernels only
    P.box_sig = (c->specialize && c->cfg.kernel_form == RTPBR_FORM_COMPLETE_PATH) ? c->scene_sig : 0;
    {
        // nearest_culled needs |sdf| to be 1-Lipschitz: true for every analytic shape except a cone whose
        // slope vector (scale.x, scale.z) is longer than 1; the rounding allowance scales with the scene
        // (the camera position counts: camera rays start there)
        float ext = 16.0f + fabsf(P.cam.lf[0]) + fabsf(P.cam.lf[1]) + fabsf(P.cam.lf[2]);
        bool ok = c->n_obj <= 8 && c->kind != KIND_BUNNY && c->kind != KIND_MIXED && ext <= 1e12f;
        for (int i = 0; i < c->n_obj; i++) {
            const ObjM& o = c->objm[i];
            const float e = fabsf(o.px) + fabsf(o.py) + fabsf(o.pz) + fabsf(o.sx) + fabsf(o.sy) + fabsf(o.sz);
            if (!(e <= 1e12f)) ok = false;
            if (e > ext) ext = e;
            if (o.type == RTPBR_SHAPE_CONE && !(o.sx * o.sx + o.sz * o.sz <= 1.0f)) ok = false;
        }
        P.cull_ok = ok ? 1 : 0;
        P.cull_extent = 4.0f * ext;
    }
    box_thresholds(c->cfg.box_round, c->lazy_sqrt, P);
    *want = false;
    *strict_error = false;
    const bool jit_bunny = c->kind == KIND_BUNNY && c->jit_bake && c->jit >= 1;   // configuration baking only (incl. which units run the network)
    const bool persistent = c->cfg.kernel_form == RTPBR_FORM_PERSISTENT_RAY;
    if (c->jit != 0 && (persistent || P.scheduler == 1) && c->n_obj <= 8 && (c->kind == KIND_BOXES || c->kind == KIND_GENERIC || (jit_bunny && !persistent))) {
        const bool aot_special = c->kind == KIND_BOXES && c->n_obj == 8 && P.box_sig != 0;
        if (c->jit >= 1 || !aot_special || c->precision) {
            *key = make_jit_key(c->kind, c->n_obj, c->objm, c->cfg, P, persistent, c->jit_bake, c->jit_waves, jit_bunny, c->precision);
            key->dense = (c->stage_dense && !persistent && !c->precision && c->noise_tracking == RTPBR_NOISE_TRACK_OFF && !c->half_mode.per_sample) ? 1 : 0;      // (a tracked or dealing launch keeps item-linear records)
            *want = true;
        }
    } else if (c->jit == 2) {
        *strict_error = true;
    }
}

static int launch_split_steps(rtpbr_ctx* c, int steps);

// What the LAST plan decided about the chain set, learned asynchronously (a 4-byte copy behind the plan kernels): the pool
// grid makes room for the chain kernel only when a plan actually produced one (advisor, round 5: the grid used to shrink
// whenever the chain kernel was merely possible — uniform-cost scenes and the launches before the first plan then ran the
// pool kernel alone on the reduced grid, measured slower: 36 against 26 ms at 768x432).
static int poll_plan_readback(rtpbr_ctx* c) {
    if (!c->plan_rb_pending) return RTPBR_OK;
    const hipError_t q = hipEventQuery(c->ev_plan_rb);
    if (q == hipSuccess) {
        c->plan_chain_waves = (int)*c->plan_rb_host;
        c->plan_rb_pending = false;
    } else if (q != hipErrorNotReady) {
        return rt_fail_hip("hipEventQuery(plan read-back)", q);
    } else {
        (void)hipGetLastError();
    }
    return RTPBR_OK;
}

// src/ persistent-ray form: n launches of pathtrace() (src/renderer.py:29-30), each cfg.steps_per_launch bounce-steps.
// A pixel's steps are sequential and the RNG is keyed by the absolute step index, so k launches of s steps equal one launch of
// k*s steps bit for bit: fuse them (<= 256 steps per kernel) instead of paying a launch + an 80 B/pixel ray_buffer round
// trip per step.  *launched: whether a kernel was enqueued (n * steps_per_launch <= 0 enqueues none; the first kernel of every
// launch zeroes the other counter buffer, P.counters_next).
static int sample_persistent(rtpbr_ctx* c, int n, bool* launched) {
    Params& P = c->P;
    long long left = (long long)n * c->cfg.steps_per_launch;
    *launched = false;
    while (left > 0) {
        int steps = (int)(left < tune::MAX_FUSED_STEPS ? left : tune::MAX_FUSED_STEPS);
        P.sample_base = c->sample_base;
        NEXT_EVENT(c->ev, c->ev_used, a);
        NEXT_EVENT(c->ev, c->ev_used, b);
        if (c->timed) HIP_TRY(hipEventRecord(a, c->stream));
        // pool scheduler unless asked otherwise: measured faster than one lane per pixel at every frame size from
        // 256x256 up (profiles/r03_src_*; round 2 switched at 2^20 pixels by a guess)
        const bool use_pool = c->scheduler != 0;
        if (use_pool) {
            const int per_cu = blocks_per_cu(c->jit_mod ? c->jit_mod->persistent_blocks_per_cu : persistent_pool_blocks_per_cu(c->kind), c->waves_per_cu);
            if (int r = poll_plan_readback(c)) return r;
            const bool chain_candidate = c->src_chain != 0 && c->grid_blocks == 0 && c->src_plan && (long long)P.np <= c->chain_np_max;
            const bool chain_room = chain_candidate && (c->plan_chain_waves > 0 || c->src_chain == 2);
            const PoolPlan pool = pool_plan(P.np, per_cu, c->n_cu, c->chain_waves, chain_candidate, chain_room, c->grid_blocks);
            P.total_items = (uint32_t)P.np;
            P.chunk = (uint32_t)c->residency;                               // bounce-steps per residency (a power of two)
            // Cost-ordered ownership: the kernel records every pixel's march steps; once plan_interval bounce-steps
            // are on record the pixels are re-ordered by them (three small kernels on the same stream) and the
            // heaviest get waves of their own.  The plan survives refresh(): what a pixel costs is a property of
            // the scene and the camera, not of the accumulated image.
            P.cost_buffer = nullptr;
            P.order = nullptr;
            P.plan = nullptr;
            P.heavy_own = c->heavy_own;
            P.heavy_prio = c->heavy_prio;
            P.src_track = c->src_track;
            P.src_op = c->src_op;
            P.leave_x8 = c->leave_x8;
            P.tiny_own = c->tiny_own;
            P.n_cu = c->n_cu;
            P.age_on = c->age_on;
            P.age_pack = 0;
            for (int k = 0; k < 8; k++) P.age_pack |= (uint32_t)(c->age_w[k] & 15) << (4 * k);
            const bool chain_eff = c->src_chain != 0 && (pool.chain_fits || c->src_chain == 2);
            if (c->src_plan) {
                if (c->plan_np != (size_t)P.np) {
                    HIP_TRY(hipStreamSynchronize(c->stream));
                    (void)hipFree(c->cost_buffer);
                    (void)hipFree(c->order);
                    c->cost_buffer = c->order = nullptr;
                    c->plan_np = 0;
                    c->order_valid = false;
                    c->cost_steps = 0;
                    c->plan_chain_waves = 0;
                    c->plan_rb_pending = false;
                    HIP_TRY(hipMalloc(&c->cost_buffer, (size_t)P.np * sizeof(uint32_t)));
                    HIP_TRY(hipMalloc(&c->order, (size_t)P.np * sizeof(uint32_t)));
                    if (!c->plan) {
                        HIP_TRY(hipMalloc(&c->plan, sizeof(PlanBuf)));
                        HIP_TRY(hipMemsetAsync(c->plan, 0, sizeof(PlanBuf), c->stream));
                    }
                    HIP_TRY(hipMemsetAsync(c->cost_buffer, 0, (size_t)P.np * sizeof(uint32_t), c->stream));
                    c->plan_np = (size_t)P.np;
                }
                if (c->cost_steps >= c->plan_interval) {
                    // (the plan sizes its heavy waves for THIS launch's grid and decides "chain-bound" against the grid the pool
                    // kernel has beside the chain kernel: the decision does not depend on whether room has been made already)
                    launch_plan(c->cost_buffer, c->order, c->plan, (uint32_t)P.np, (uint32_t)pool.grid * 4u, c->heavy_own, c->heavy_mean_x16,
                                c->heavy_bulk_x16, c->tiny_waves, c->n_cu, pool.n_cls, chain_candidate || c->src_chain == 2 ? c->chain_waves : 0,
                                (uint32_t)pool.grid_room * 4u, c->stream);
                    c->order_valid = true;
                    c->cost_steps = 0;
                    if (!c->plan_rb_host) {
                        HIP_TRY(hipHostMalloc((void**)&c->plan_rb_host, 64, hipHostMallocDefault));
                        HIP_TRY(hipEventCreateWithFlags(&c->ev_plan_rb, hipEventDisableTiming));
                    }
                    HIP_TRY(hipMemcpyAsync(c->plan_rb_host, &c->plan->n_chain_waves, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
                    HIP_TRY(hipEventRecord(c->ev_plan_rb, c->stream));
                    c->plan_rb_pending = true;
                }
                P.cost_buffer = c->cost_buffer;
                P.order = c->order_valid ? c->order : nullptr;
                P.plan = c->plan;
                c->cost_steps += steps;
            }
            if (c->src_split > 0 && steps <= c->src_split) {
                if (int r = launch_split_steps(c, steps)) return r;
            } else {
                if (int r = flush_shade(c)) return r;
                // A chain-bound launch hands the head of the cost-ordered list to the chain kernel (rt_chain.hpp), which runs
                // BESIDE the pool kernel on a second stream: forked after the plan, joined before anything else touches the
                // buffers.  Its grid covers the largest chain set a plan can make; waves without an entry leave at once.
                P.chain_on = (chain_eff && P.order) ? 1 : 0;
                bool forked = false;
                int rc = RTPBR_OK;
                if (P.chain_on) {
                    if (!c->stream2) {
                        HIP_TRY(hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking));
                        HIP_TRY(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
                        HIP_TRY(hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
                    }
                    HIP_TRY(hipEventRecord(c->ev_fork, c->stream));
                    HIP_TRY(hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
                    forked = true;
                    if (c->jit_mod)
                        rc = rt_jit_launch_steps(c->jit_mod->chain_steps, P, steps, (unsigned)tune::CHAIN_GRID_BLOCKS, c->stream2);
                    else
                        launch_chain_steps(P, c->kind, steps, tune::CHAIN_GRID_BLOCKS, c->stream2);
                }
                if (rc == RTPBR_OK) {
                    if (c->jit_mod)
                        rc = rt_jit_launch_steps(c->jit_mod->persistent_pool, P, steps, (unsigned)pool.grid, c->stream);
                    else
                        launch_persistent_pool(P, c->kind, steps, (int)pool.grid, c->stream);
                }
                // JOIN on every exit once the second stream has been forked (advisor, round 5): nothing that follows on the
                // context's stream may overtake a chain kernel that is still running — if the event cannot be recorded, wait
                // for the stream itself
                if (forked) {
                    if (hipEventRecord(c->ev_join, c->stream2) != hipSuccess || hipStreamWaitEvent(c->stream, c->ev_join, 0) != hipSuccess) {
                        (void)hipGetLastError();
                        (void)hipStreamSynchronize(c->stream2);
                    }
                }
                P.chain_on = 0;      // (persistent state of the context: only this launch ran with the chain set split off)
                if (rc != RTPBR_OK) return rc;
            }
        } else if (c->jit_mod) {
            if (int r = rt_jit_launch_steps(c->jit_mod->persistent_steps, P, steps, (unsigned)((P.np + 255) / 256), c->stream)) return r;
        } else {
            if (int r = flush_shade(c)) return r;
            launch_persistent(P, c->kind, steps, c->stream);
        }
        if (c->timed) HIP_TRY(hipEventRecord(b, c->stream));
        *launched = true;
        c->sample_base += (uint32_t)steps;
        left -= steps;
    }
    return RTPBR_OK;
}

// A launch of one (or a few) bounce-steps — the way the reference calls pathtrace(), src/renderer.py:29-30 — as the wavefront
// split of rt_split.hpp: per step gen (roulette / deposit / camera ray), march (the raycasts, heaviest first from the
// cost-ordered list), shade.  Same results, same counters as the fused kernels.
static int launch_split_steps(rtpbr_ctx* c, int steps) {
    Params& P = c->P;
    if (c->march_np != (size_t)P.np) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        (void)hipFree(c->march_out);
        c->march_out = nullptr;
        c->march_np = 0;
        HIP_TRY(hipMalloc(&c->march_out, (size_t)P.np * sizeof(uint32_t)));
        c->march_np = (size_t)P.np;
    }
    P.march_out = c->march_out;
    P.wait_lanes = c->split_wait;
    P.chain_on = 0;
    const MarchPlan march = march_plan(P.np, c->jit_mod ? c->jit_mod->march_blocks_per_cu : src_march_blocks_per_cu(c->kind), c->n_cu, c->waves_per_cu,
                                       c->grid_blocks, c->split_head, c->sparse_lanes, c->src_op, c->n_obj);
    const int sparse_saved = P.sparse_lanes;
    P.sparse_lanes = march.sparse_lanes;
    P.split_head = march.split_head;
    P.team_counter = c->team_counter;
    P.n_teams = march.n_teams;
    int rc = RTPBR_OK;
    // lazy shading: a step's shading rides with the next step's gen pass (src_shade_gen) — flush_shade() launches it when something
    // else wants to see ray_buffer or the counters first
    const bool lazy = c->src_lazy != 0 && !c->ray_ptr_out;
    for (int i = 0; i < steps && rc == RTPBR_OK; i++) {
        P.sample_base = c->sample_base + (uint32_t)i;
        const bool shade_first = c->shade_pending, count = c->shade_pending_same_call;
        if (shade_first) {
            P.shade_base = c->shade_pending_base;
            c->shade_pending = false;
        }
        if (c->jit_mod) {
            rc = rt_jit_launch(!shade_first ? c->jit_mod->src_gen : count ? c->jit_mod->src_shade_gen_count : c->jit_mod->src_shade_gen, P, (unsigned)march.need, c->stream);
            if (rc == RTPBR_OK) rc = rt_jit_launch(c->jit_mod->src_march, P, (unsigned)march.grid, c->stream);
            if (rc == RTPBR_OK && !lazy) rc = rt_jit_launch(c->jit_mod->src_shade, P, (unsigned)march.need, c->stream);
        } else {
            if (shade_first) launch_src_shade_gen(P, c->kind, count, c->stream);
            else launch_src_gen(P, c->kind, c->stream);
            launch_src_march(P, c->kind, (int)march.grid, c->stream);
            if (!lazy) launch_src_shade(P, c->kind, c->stream);
        }
        if (lazy && rc == RTPBR_OK) {
            c->shade_pending = true;
            c->shade_pending_base = P.sample_base;
            c->shade_pending_same_call = true;
        }
    }
    P.sparse_lanes = sparse_saved;
    return rc;
}

// complete-path form: `n` samples per owned pixel (the spp loop of cornell_box_v3/renderer.py:31-36), in sub-launches of as
// many samples per pixel as the staging budget holds.  `selected` (rtpbr_sample_selected): the caller has set P.np to the selection
// list's length (> 0) and P.order to the list — the general ahead-of-time instances with the list indirection, item-linear staging,
// no primary split, no run-time instance (c->jit_mod is nullptr, P.box_sig 0).  `fresh` is false for the later stages of a tiered
// selected call (sample_selected_tiered): the call's first sub-launch was an earlier stage's.
static int sample_complete_path(rtpbr_ctx* c, int n, bool selected = false, bool fresh = true) {
    Params& P = c->P;
    int left = n;
    if (int r = flush_shade(c)) return r;
    if (fresh) c->dense_launches = 0;
    // per-sample noise tracking (rtpbr_set_noise_tracking): the accumulate pass folds every record into the moments (the callers
    // have refused what keeps no records and have allocated the moments and the snapshot)
    const bool tracked = c->noise_tracking == RTPBR_NOISE_TRACK_SAMPLES;
    // per-sample dealing to the halves (rtpbr_set_half_mode): likewise, into half A and its snapshot
    const bool dealt = c->half_mode.per_sample != 0;
    while (left > 0) {
        const bool split_ok = !selected && c->primary_split && P.scheduler == 1 && c->kind != KIND_BUNNY && c->kind != KIND_MIXED;
        // the tolerance flavour accumulates in LDS and adds to image_buffer directly: no staging, no accumulate kernel
        const bool unstaged = c->precision != 0 && c->jit_mod != nullptr && P.scheduler == 1;
        const StagingPlan sp = staging_plan(P.np, left, c->staging_bytes, c->n_cu, split_ok, unstaged, c->primary_split);
        const int K = (int)sp.K;
        const bool split = sp.split;
        if (int r = ensure_staging(c, (size_t)P.np * (size_t)K, split, !unstaged)) {
            // no room for K samples per launch: halve the budget and go round again (1 spp per launch must fit)
            if (r != RTPBR_ENOMEM || K == 1)
                return r == RTPBR_ENOMEM ? fail(RTPBR_ENOMEM, "no device memory for the staging of one sample per pixel") : r;
            c->staging_bytes = (long long)((K + 1) / 2) * sp.per_spp;
            continue;
        }
        P.primary = c->primary;
        P.primary_code = reinterpret_cast<uint8_t*>(c->primary + (size_t)P.np * (size_t)K);
        P.primary_split = split ? 1 : 0;
        P.primary_lean = c->primary_lean;
        P.drain_lanes = c->drain_lanes;
        P.stage = c->stage;
        P.K = K;
        P.k_shift = item_shift_of(K);       // (rt_item.hpp: a power-of-two K splits the work item by shift and mask)
        P.sample_base = c->sample_base;
        P.total_items = sp.total_items;
        const int grid = trace_grid(c, P.total_items, selected);
        const long long chunk = claim_plan(P.total_items, grid, c->chunk);
        P.chunk = (uint32_t)chunk;
        P.stage_dense = 0;
        if (c->stage_dense && c->jit_mod != nullptr && !unstaged && P.scheduler == 1 && !tracked && !dealt) {      // (compiled into run-time instances only: RtJitKey::dense)
            const DensePlan dense = dense_plan(P.total_items, K, chunk, c->chunk);
            if (dense.on) {
                P.chunk = dense.chunk;
                P.stage_dense = 1;
                c->dense_launches++;
                P.acc_batch = dense.acc_batch;
                P.acc_magic_k = dense.acc_magic_k;
                P.acc_magic_chunk = dense.acc_magic_chunk;
                P.stage_fill = reinterpret_cast<uint32_t*>(c->stage + (size_t)P.total_items * 3u);
                P.stage_idx = reinterpret_cast<uint8_t*>(P.stage_fill + dense.n_fill);
                HIP_TRY(hipMemsetAsync(P.stage_fill, 0, dense.n_fill * sizeof(uint32_t), c->stream));
            }
        }
        // [0] trace items, [1] primary groups: zeroed with the work counters by rtpbr_sample(); again before every further sub-launch
        if (left != n || !fresh) launch_zero(c->work_counter, 64, c->stream);
        if (split) {
            NEXT_EVENT(c->evp, c->evp_used, pa);
            NEXT_EVENT(c->evp, c->evp_used, pb);
            if (c->timed) HIP_TRY(hipEventRecord(pa, c->stream));
            if (c->jit_mod) {
                if (int r = rt_jit_launch(c->jit_mod->primary, P, (unsigned)capped_grid(tune::PRIMARY_BLOCKS_PER_CU, c->n_cu, P.total_items), c->stream)) return r;
            } else
                launch_primary(P, c->kind, c->n_cu, c->stream);
            if (c->timed) HIP_TRY(hipEventRecord(pb, c->stream));
        }
        NEXT_EVENT(c->ev, c->ev_used, a);
        NEXT_EVENT(c->ev, c->ev_used, b);
        if (c->timed) HIP_TRY(hipEventRecord(a, c->stream));
        if (selected) {
            launch_trace_selected(P, c->kind, grid, c->stream);
        } else if (c->jit_mod) {
            if (int r = rt_jit_launch(c->jit_mod->trace, P, (unsigned)grid, c->stream)) return r;
        } else
            launch_trace(P, c->kind, grid, c->stream);
        if (c->timed) HIP_TRY(hipEventRecord(b, c->stream));
        float4* const mo = tracked ? c->noise_moments : nullptr;
        if (dealt && selected) launch_accumulate_selected_dealt(P, mo, c->noise_snapshot, c->half_a, c->half_snapshot, c->stream);
        else if (dealt) launch_accumulate_dealt(P, mo, c->noise_snapshot, c->half_a, c->half_snapshot, c->stream);
        else if (tracked && selected) launch_accumulate_selected_tracked(P, c->noise_moments, c->noise_snapshot, c->stream);
        else if (tracked) launch_accumulate_tracked(P, c->noise_moments, c->noise_snapshot, c->stream);
        else if (selected) launch_accumulate_selected(P, c->stream);
        else if (!unstaged) launch_accumulate(P, c->n_cu, c->stream);
        c->sample_base += (uint32_t)K;
        left -= K;
    }
    return RTPBR_OK;
}

// rtpbr_sample_selected(n) on a tiered selection (T = c->sel_tiers > 1; include/rtpbr.h): with the shares s_t = max(1, n >> t),
// s_T = 0, stage t = T-1 .. 0 traces the sample indices base + s_{t+1} .. base + s_t - 1 through the first L_t entries of the list
// (the pixels of tiers 0 .. t) — an ordinary selected launch each, P.np = L_t, the context's sample_base set for the stage.  The index
// ranges ascend from stage to stage, so every pixel's records are added in sample order; a tier-t pixel skips s_t .. n - 1.
// The caller has set P.order to the list and puts P.np back.
static int sample_selected_tiered(rtpbr_ctx* c, int n) {
    const uint32_t base = c->sample_base;
    const int T = c->sel_tiers;
    if (int r = flush_shade(c)) return r;
    c->dense_launches = 0;
    bool fresh = true;
    for (int t = T - 1; t >= 0 && n > 0; t--) {
        const TierStage st = tier_stage(n, t, T);
        if (st.hi == st.lo || c->sel_cum[t] == 0) continue;
        c->P.np = (int32_t)c->sel_cum[t];
        c->sample_base = base + (uint32_t)st.lo;
        if (int r = sample_complete_path(c, st.hi - st.lo, true, fresh)) return r;
        fresh = false;
    }
    c->sample_base = base + (uint32_t)n;
    return RTPBR_OK;
}

// rtpbr_sample and rtpbr_sample_selected (`selected`: every refusal of its own has been made by the caller)
static int sample_call(rtpbr_ctx* c, int n, bool selected) {
    if (int r = set_dev(c)) return r;
    // (diff_buffer: instrumented builds write their per-wave records over it; a tracked call — rtpbr_set_noise_tracking — writes the moments)
    const bool tracked = c->noise_tracking == RTPBR_NOISE_TRACK_SAMPLES;
    const bool dealt = c->half_mode.per_sample != 0;      // ... and a dealing call — rtpbr_set_half_mode — half A
    if (int r = rt_order_after_reads(c, W_IMAGE_BUFFER | W_RAY_BUFFER | W_DIFF_BUFFER | (tracked ? W_MOMENTS : 0u) | (dealt ? W_HALF : 0u))) return r;
    // A shading the previous call left pending (lazy shading of one-step launches) rides along only if this call is again a launch of the
    // wavefront split; otherwise it is launched now, while the previous call's work counters are still the current ones
    {
        const long long steps = (long long)n * c->cfg.steps_per_launch;
        const bool split_again = c->cfg.kernel_form == RTPBR_FORM_PERSISTENT_RAY && c->scheduler != 0 && c->src_split > 0 && steps >= 1 &&
                                 steps <= c->src_split && c->src_lazy != 0 && !c->ray_ptr_out;
        if (!split_again)
            if (int r = flush_shade(c)) return r;
        c->shade_pending_same_call = false;
    }
    Params& P = c->P;
    RtJitKey key{};
    bool want_jit = false, strict_error = false;
    derive_launch(c, &key, &want_jit, &strict_error);
    // A run-time compiled instance of THIS scene (rt_jit.hip), when no listed ahead-of-time signature serves it
    rt_jit_release(c->jit_mod);
    c->jit_mod = nullptr;
    if (selected) {
        // a selected launch runs the general ahead-of-time instances (rt_kernels.hip launch_trace_selected), whatever the jit,
        // jit_bake and specialize options say: same bits (the next rtpbr_sample derives its own instance again)
        P.box_sig = 0;
    } else if (want_jit) {
        RtJitModule* jm = nullptr;
        const int r = rt_jit_acquire(c, key, &jm);
        if (r == RTPBR_OK) {
            c->jit_mod = jm;
            P.box_sig = key.sig;
        } else if (c->jit == 2) {
            return r;
        }
    } else if (strict_error) {
        return fail(RTPBR_ESTATE, "option jit = 2 (strict): no run-time instance exists for this scene (needs <= 8 analytic shapes, "
                                  "or the neural shape with jit_bake, and the pool scheduler)");
    }
    if (c->precision && !c->jit_mod && !selected)
        return fail(RTPBR_ESTATE, "option precision = 1 (the tolerance flavour) exists as a run-time compiled instance only: needs hipcc and the kernel "
                                  "sources on this machine, option jit != 0, a scene of <= 8 analytic shapes (or the neural shape with jit_bake = 1, jit >= 1) "
                                  "and the pool scheduler");
    pack_objects(c, P);
    for (int i = 0; i < c->n_obj; i++)
        if (c->obj[i].type == RTPBR_SHAPE_BUNNY && !c->bunny) return fail(RTPBR_ESTATE, "bunny shape needs rtpbr_set_shape_data first");
    if (c->cfg.sky_kind == RTPBR_SKY_ENVMAP && !c->env) return fail(RTPBR_ESTATE, "sky_kind ENVMAP needs rtpbr_set_env first");
    // a tracked call folds into the moments and re-takes the snapshot: both exist (zeroed) from here on, as after rtpbr_noise_update
    if (tracked)
        if (int r = frame_need(c, {ROW_noise_moments, ROW_noise_snapshot})) return r;
    // a dealing call deals into half A and re-takes its snapshot: both exist (zeroed) from here on, as after rtpbr_half_update
    if (dealt)
        if (int r = frame_need(c, {ROW_half_a, ROW_half_snapshot})) return r;
    static_assert((sizeof(Counters) + 64) % 16 == 0, "zero_next_counters / launch_zero fill 16-byte words");
    // This call's work counters (+ the claim counters behind them): the buffer whose turn it is, zeroed by the previous call's kernels
    // (or here, if that call launched none); this call's kernels zero the other one.
    const int turn = c->counters_turn;
    c->counters = c->counters_buf[turn];
    c->work_counter = reinterpret_cast<unsigned int*>(reinterpret_cast<char*>(c->counters) + sizeof(Counters));
    if (!c->counters_clean[turn]) launch_zero(c->counters, sizeof(Counters) + 64, c->stream);
    P.counters = c->counters;
    P.work_counter = c->work_counter;
    P.counters_next = c->cfg.kernel_form == RTPBR_FORM_PERSISTENT_RAY ? c->counters_buf[turn ^ 1] : nullptr;
    c->counters_clean[turn] = false;
    c->counters_clean[turn ^ 1] = false;
    c->counters_turn = turn ^ 1;
    c->ev_used = 0;
    c->evp_used = 0;
    c->timed = c->timing != 0;
    c->total1_recorded = false;
    bool zeroed_next = false;
    if (selected) {
        // the work geometry of the list for this call only: the context's own comes back for later full-frame calls
        const int32_t np_keep = P.np;
        const uint32_t* const order_keep = P.order;
        int r = RTPBR_OK;
        if (c->sel_count > 0) {
            P.np = (int32_t)c->sel_count;
            P.order = c->sel_list;
            r = c->sel_tiers > 1 ? sample_selected_tiered(c, n) : sample_complete_path(c, n, true);
            P.np = np_keep;
            P.order = order_keep;
        } else {
            r = flush_shade(c);
            c->dense_launches = 0;
            c->sample_base += (uint32_t)n;      // the unselected pixels skip these indices: here that is all of them
        }
        if (r) return r;
    } else if (c->cfg.kernel_form == RTPBR_FORM_PERSISTENT_RAY) {
        if (int r = sample_persistent(c, n, &zeroed_next)) return r;
    } else {
        if (int r = sample_complete_path(c, n)) return r;
    }
    // (the call's first event doubles as its start; an end event of its own only where work follows the last timed kernel: every event
    // is ~4 us of idle queue between two small kernels)
    if (c->timed && c->cfg.kernel_form != RTPBR_FORM_PERSISTENT_RAY) {
        HIP_TRY(hipEventRecord(c->ev_total1, c->stream));
        c->total1_recorded = true;
    }
    HIP_TRY(hipGetLastError());
    // (the first kernel of every src/ path zeroed the other buffer: persistent pool / persistent steps / src_gen; a persistent-ray call
    // of no bounce-steps — n = 0 or steps_per_launch <= 0 — enqueued none, and the complete-path kernels zero nothing)
    c->counters_clean[c->counters_turn] = zeroed_next;
    return RTPBR_OK;
}

// what a sample call with per-sample noise tracking (rtpbr_set_noise_tracking) or per-sample dealing (rtpbr_set_half_mode) on refuses:
// there must be a record per sample
static int tracked_sample_check(rtpbr_ctx* c) {
    if (c->half_mode.per_sample) {      // rtpbr_set_half_mode: the same three refusals
        if (c->cfg.kernel_form != RTPBR_FORM_COMPLETE_PATH)
            return fail(RTPBR_ESTATE, "per-sample dealing to the halves: the complete-path form only (the persistent-ray form has no per-sample records): "
                                      "rtpbr_set_half_mode with per_sample = 0 first");
        if (c->precision)
            return fail(RTPBR_ESTATE, "per-sample dealing to the halves: not with option precision = 1 (the tolerance flavour's unstaged instance keeps no records)");
        if (c->world > 1) return fail(RTPBR_ESTATE, "per-sample dealing to the halves works on the whole frame: not with tiles of world > 1");
    }
    if (c->noise_tracking != RTPBR_NOISE_TRACK_SAMPLES) return RTPBR_OK;
    if (c->cfg.kernel_form != RTPBR_FORM_COMPLETE_PATH)
        return fail(RTPBR_ESTATE, "per-sample noise tracking: the complete-path form only (the persistent-ray form has no per-sample records): "
                                  "rtpbr_set_noise_tracking(RTPBR_NOISE_TRACK_OFF) first");
    if (c->precision)
        return fail(RTPBR_ESTATE, "per-sample noise tracking: not with option precision = 1 (the tolerance flavour's unstaged instance keeps no records)");
    if (c->world > 1) return fail(RTPBR_ESTATE, "per-sample noise tracking works on the whole frame: not with tiles of world > 1");
    return RTPBR_OK;
}

extern "C" int rtpbr_sample(rtpbr_ctx* c, int n) {
    if (!c) return fail(RTPBR_EINVAL, "null ctx");
    if (!c->have_cfg || !c->have_scene || !c->have_cam) return fail(RTPBR_ESTATE, "set_config, set_scene and set_camera first");
    if (n < 0) return fail(RTPBR_EINVAL, "n must be >= 0");
    if (int r = tracked_sample_check(c)) return r;
    return sample_call(c, n, false);
}

extern "C" int rtpbr_post_process(rtpbr_ctx* c) {
    if (!c || !c->have_cfg) return fail(RTPBR_ESTATE, "set_config first");
    if (int r = set_dev(c)) return r;
    if (int r = rt_order_after_reads(c, W_IMAGE_PIXELS | W_DIFF_BUFFER | W_DIFF_PIXELS)) return r;
    c->P.cfg = c->cfg;
    c->P.image_buffer = c->image_buffer;
    c->P.image_pixels = c->image_pixels;
    c->P.diff_buffer = c->diff_buffer;
    c->P.diff_pixels = c->diff_pixels;
    launch_post_process(c->P, c->stream);
    HIP_TRY(hipGetLastError());
    return RTPBR_OK;
}

// ---- first-hit features and the a-trous denoise (rt_features.hip): the filter the reference's post_process() leaves as a TODO
// (src/postprocessor.py:30 "# ToDo: Post Denoise").  Whole-frame only: a rank of a tiled render holds part of the frame.

// The states every call on the whole frame refuses, in this order: no configuration, scene or camera yet; tiles of world > 1
// (`tiles`: the call's message, `who` fills its %s if it has one); a bunny without its shape data.
static int whole_frame_state(rtpbr_ctx* c, const char* tiles, const char* who = "") {
    if (!c->have_cfg || !c->have_scene || !c->have_cam) return fail(RTPBR_ESTATE, "set_config, set_scene and set_camera first");
    if (c->world > 1) return fail(RTPBR_ESTATE, tiles, who);
    for (int i = 0; i < c->n_obj; i++)
        if (c->obj[i].type == RTPBR_SHAPE_BUNNY && !c->bunny) return fail(RTPBR_ESTATE, "bunny shape needs rtpbr_set_shape_data first");
    return RTPBR_OK;
}
static const char* const FEATURE_TILES = "rtpbr_render_features / rtpbr_denoise work on the whole frame: not with tiles of world > 1";

// The Params of the feature rays at g x g rays per pixel (g = 1: rtpbr_render_features; the sub-rays of the coverage plane are the
// feature rays of the g-fold configuration): the context's, with that width, height and their reciprocals and the general march
// table (signature 0, no lazy box keys), which is what the run-time object-count instances read
static Params feature_params(rtpbr_ctx* c, int g) {
    Params P = c->P;
    P.cfg = c->cfg;
    P.cfg.width = g * c->cfg.width;
    P.cfg.height = g * c->cfg.height;
    P.cam.inv_w = 1.0f / (float)P.cfg.width;
    P.cam.inv_h = 1.0f / (float)P.cfg.height;
    P.n_obj = c->n_obj;
    P.box_sig = 0;
    P.box_lazy = 0;
    pack_table(c->objm, c->n_obj, 0, P.objm);
    P.objfull = c->objfull;
    P.bunny = c->bunny;
    return P;
}

extern "C" int rtpbr_render_features(rtpbr_ctx* c) {
    if (!c) return fail(RTPBR_EINVAL, "null ctx");
    if (int r = whole_frame_state(c, FEATURE_TILES)) return r;
    if (int r = set_dev(c)) return r;
    if (int r = frame_need(c, {ROW_feat_albedo, ROW_feat_normal, ROW_feat_depth, ROW_feat_object, ROW_feat_guides})) return r;
    if (int r = rt_order_after_reads(c, W_FEATURES)) return r;
    const Params P = feature_params(c, 1);
    FeatArgs A;
    A.albedo = c->feat_albedo;
    A.normal = c->feat_normal;
    A.depth = c->feat_depth;
    A.object = c->feat_object;
    A.guide_nz = c->feat_guides;
    launch_features(P, A, c->kind, c->stream);
    HIP_TRY(hipGetLastError());
    c->feat_valid = true;
    c->cov_valid = false;      // (built from the features that were)
    return RTPBR_OK;
}

// iterations, demodulate and the sigmas (sig[0]: sigma_color) of either denoise call; inv[k] = 1 / sig[k]^2
static int denoise_params_check(int iterations, int demodulate, const float* sig, float* inv, int n_sig) {
    if (iterations < 0 || iterations > 8) return fail(RTPBR_EINVAL, "denoise iterations must be 0..8");
    if (demodulate != 0 && demodulate != 1) return fail(RTPBR_EINVAL, "denoise demodulate must be 0 or 1");
    for (int k = 0; k < n_sig; k++) {
        inv[k] = 1.0f / (sig[k] * sig[k]);
        if (!(sig[k] > 0.0f) || !std::isfinite(sig[k]) || !std::isfinite(inv[k]))
            return fail(RTPBR_EINVAL, "denoise sigmas must be finite and > 0 (and not so small that 1/sigma^2 overflows)");
    }
    return RTPBR_OK;
}

// the two halves of a chain's ping-pong: from two levels on
static int denoise_scratch_need(rtpbr_ctx* c, int iterations) { return iterations >= 2 ? frame_need(c, {ROW_denoise_scratch}) : RTPBR_OK; }

// RTPBR_BUF_DENOISED_PIXELS and the ping-pong; then ordered after the buffer's reads
static int denoised_alloc(rtpbr_ctx* c, int iterations) {
    if (int r = set_dev(c)) return r;
    if (int r = frame_need(c, {ROW_denoised})) return r;
    if (int r = denoise_scratch_need(c, iterations)) return r;
    return rt_order_after_reads(c, W_DENOISED);
}

// what every a-trous launch of a call shares; the level's buffers, step and colour weight are the caller's
static DenoiseArgs denoise_args(rtpbr_ctx* c, int demodulate, const float* inv) {
    DenoiseArgs A{};
    A.cfg = c->cfg;
    A.guide_nz = c->feat_guides;
    A.albedo = c->feat_albedo;
    A.object = c->feat_object;
    A.in = inv[1];
    A.iz = inv[2];
    A.demodulate = demodulate;
    A.width = c->cfg.width;
    A.height = c->cfg.height;
    return A;
}

// The shards the filling kernels count into, zeroed on the stream: the call's own (what counters "fill_*" read), and behind them a
// second set nobody reads (the half chains of the level blend with option blend_fill = 1 count there).
constexpr size_t FILL_COUNT_WORDS = (size_t)FILL_SHARDS * FILL_SHARD_WORDS;
static int fill_counts_zero(rtpbr_ctx* c) {
    constexpr size_t bytes = 2 * FILL_COUNT_WORDS * sizeof(uint32_t);
    if (!c->fill_counts) HIP_TRY(hipMalloc(&c->fill_counts, bytes));
    HIP_TRY(hipMemsetAsync(c->fill_counts, 0, bytes, c->stream));
    return RTPBR_OK;
}

// a launcher found no instance for the form it was asked for and launched nothing (no call of include/rtpbr.h asks for one)
static int no_instance(const char* family) { return fail(RTPBR_EHIP, "internal error: no instance of %s for the form asked for", family); }

// where level k of `levels` stands, and the level in A: its step 2^k, the plain filter's colour weight and the ping-pong.  The level
// reads plane (k - 1) & 1 of `planes` (n records each; not at LEVEL_FIRST, which reads A.image_buffer) and writes plane k & 1 (not at
// LEVEL_LAST, which writes A.out).  variance: the guided filter's two planes (its colour weight is per pixel), which go the same way
static unsigned level_position(int k, int levels) { return (k == 0 ? LEVEL_FIRST : 0u) | (k + 1 == levels ? LEVEL_LAST : 0u); }
static void level_args(DenoiseArgs& A, int k, unsigned position, const float* inv, float4* planes, float* variance, size_t n) {
    const bool first = (position & LEVEL_FIRST) != 0, last = (position & LEVEL_LAST) != 0;
    const size_t before = (size_t)((k - 1) & 1) * n, now = (size_t)(k & 1) * n;
    A.src = first ? nullptr : planes + before;
    A.dst = last ? nullptr : planes + now;
    if (variance) {
        A.vsrc = first ? nullptr : variance + before;
        A.vdst = last ? nullptr : variance + now;
    } else {
        A.ic = inv[0] * (float)(1u << (2 * k));     // sigma_c halves at every level (exact: a power of two)
    }
    A.step = 1 << k;
}

// One run of the filter.  The calls that run the same filter on several buffers build it once and vary in and out.
struct FilterChain {
    const float4* in = nullptr;       // the (sum r, sum g, sum b, count) buffer; nullptr: image_buffer
    float* out = nullptr;             // the last level's (W,H,3) plane; nullptr: RTPBR_BUF_DENOISED_PIXELS, allocated here with the ping-pong
    unsigned form = 0;                // ATROUS_LINEAR (with out); ATROUS_FILL (iterations > 0): the levels count into fill_counts, zeroed first
    const rtpbr_denoise_guided_params* guided = nullptr;      // ATROUS_GUIDED: the variance goes through noise_var's planes 1 and 2
    const float* cover_k = nullptr;   // ATROUS_COVER (with ATROUS_LINEAR, iterations > 0); with ATROUS_FILL the last level writes cov_live
    FilterChain on(const float4* in_, float* out_) const { return FilterChain{in_, out_, form, guided, cover_k}; }
};

// The levels of a chain, after every refusal, through the two halves of denoise_scratch.  No level: the tone-map-only pass
static int denoise_levels(rtpbr_ctx* c, int iterations, int demodulate, const float* inv, const FilterChain& ch) {
    if (!ch.out)
        if (int r = denoised_alloc(c, iterations)) return r;
    const size_t n = (size_t)c->cfg.width * c->cfg.height;
    const unsigned form = ch.form | (ch.guided ? ATROUS_GUIDED : 0u) | (ch.cover_k ? ATROUS_COVER : 0u);
    DenoiseArgs A = denoise_args(c, demodulate, inv);
    A.image_buffer = ch.in ? ch.in : c->image_buffer;
    A.out = ch.out ? ch.out : c->denoised;
    if (ch.cover_k) A.cover_k = ch.cover_k;      // (shares var0's word: never with guided)
    if (form & ATROUS_FILL) {
        if (int r = fill_counts_zero(c)) return r;
        A.fill = c->fill_counts;                 // (shares vsrc's word: never with guided)
        if (ch.cover_k) A.live = c->cov_live;    // (shares vdst's word: never with guided)
    }
    if (ch.guided) {
        A.var0 = c->noise_var;
        A.sc2 = ch.guided->sigma_color * ch.guided->sigma_color;
        A.floor = ch.guided->variance_floor;
    }
    if (iterations == 0 && !launch_atrous_level(A, LEVEL_ONLY | form, c->stream)) return no_instance("atrous_level");      // (A.step = 0)
    for (int k = 0; k < iterations; k++) {
        const unsigned position = level_position(k, iterations);
        level_args(A, k, position, inv, c->denoise_scratch, ch.guided ? c->noise_var + n : nullptr, n);
        if (!launch_atrous_level(A, position | form, c->stream)) return no_instance("atrous_level");
    }
    HIP_TRY(hipGetLastError());
    return RTPBR_OK;
}

// p (NULL: the defaults) -> d and inv[k] = 1 / sigma_k^2, after the parameter checks of rtpbr_denoise
static int denoise_params(const rtpbr_denoise_params* p, rtpbr_denoise_params& d, float* inv) {
    if (p) {
        d = *p;
    } else {
        d.iterations = RTPBR_DENOISE_DEFAULT_ITERATIONS;
        d.demodulate = RTPBR_DENOISE_DEFAULT_DEMODULATE;
        d.sigma_color = RTPBR_DENOISE_DEFAULT_SIGMA_COLOR;
        d.sigma_normal = RTPBR_DENOISE_DEFAULT_SIGMA_NORMAL;
        d.sigma_depth = RTPBR_DENOISE_DEFAULT_SIGMA_DEPTH;
        d.sigma_albedo = RTPBR_DENOISE_DEFAULT_SIGMA_ALBEDO;
    }
    const float sig[4] = {d.sigma_color, d.sigma_normal, d.sigma_depth, d.sigma_albedo};
    if (int r = denoise_params_check(d.iterations, d.demodulate, sig, inv, 4)) return r;
    // the colour weight alone grows, by 4 per level: it must stay finite up to the last level, 4^(iterations-1)
    if (d.iterations > 1 && !std::isfinite(inv[0] * (float)(1u << (2 * (d.iterations - 1)))))
        return fail(RTPBR_EINVAL, "denoise sigma_color too small for this many levels: 1/sigma^2 * 4^(iterations-1) overflows");
    return RTPBR_OK;
}

extern "C" int rtpbr_denoise(rtpbr_ctx* c, const rtpbr_denoise_params* p) {
    if (!c) return fail(RTPBR_EINVAL, "null ctx");
    rtpbr_denoise_params d;
    float inv[4];
    if (int r = denoise_params(p, d, inv)) return r;
    if (int r = whole_frame_state(c, FEATURE_TILES)) return r;
    if (!c->feat_valid)
        if (int r = rtpbr_render_features(c)) return r;
    // option denoise_fill: the filling levels (iterations = 0 has no level: nothing is filled, the counters keep the last filling call's)
    FilterChain ch;
    if (c->denoise_fill && d.iterations > 0) ch.form = ATROUS_FILL;
    return denoise_levels(c, d.iterations, d.demodulate, inv, ch);
}

// ---- sub-pixel coverage and the coverage-aware denoise (rt_coverage.hip)

// v (NULL: the defaults) -> d, after the parameter checks of the two coverage calls
static int coverage_params(const rtpbr_coverage_params* v, rtpbr_coverage_params& d) {
    static_assert(sizeof(rtpbr_coverage_params) == 12, "three 4-byte members");
    d = v ? *v : rtpbr_coverage_params{RTPBR_COVERAGE_DEFAULT_GRID, RTPBR_COVERAGE_DEFAULT_POWER, RTPBR_COVERAGE_DEFAULT_RESOLVE};
    if (d.grid != 2 && d.grid != 4) return fail(RTPBR_EINVAL, "coverage grid must be 2 or 4");
    if (d.power < 0 || d.power > 8) return fail(RTPBR_EINVAL, "coverage power must be 0..8");
    if (d.resolve != 0 && d.resolve != 1) return fail(RTPBR_EINVAL, "coverage resolve must be 0 or 1");
    return RTPBR_OK;
}

static CoverageArgs coverage_args(rtpbr_ctx* c, const rtpbr_coverage_params& d) {
    CoverageArgs A{};
    A.object = c->feat_object;
    A.coverage = c->coverage;
    A.list = c->cov_list;
    A.k = c->cov_k;
    A.width = c->cfg.width;
    A.height = c->cfg.height;
    A.grid = d.grid;
    A.power = d.power;
    return A;
}

// The coverage plane at grid d.grid on the stream, unless it is there already; after whole_frame_state; sets the device.
static int coverage_enqueue(rtpbr_ctx* c, const rtpbr_coverage_params& d) {
    if ((long long)d.grid * c->cfg.width > 65535 || (long long)d.grid * c->cfg.height > 65535)
        return fail(RTPBR_EINVAL, "coverage: grid x resolution out of range (1..65535)");
    if (int r = set_dev(c)) return r;
    if (!c->feat_valid)
        if (int r = rtpbr_render_features(c)) return r;
    if (c->cov_valid && c->cov_rendered_grid == d.grid) return RTPBR_OK;
    if (int r = frame_need(c, {ROW_coverage, ROW_cov_list})) return r;
    const CoverageArgs A = coverage_args(c, d);
    HIP_TRY(hipMemsetAsync(c->cov_list, 0, COVER_HEAD * sizeof(uint32_t), c->stream));
    launch_cover_mark(A, c->stream);
    launch_cover_rays(feature_params(c, d.grid), A, c->kind, c->n_cu, c->cover_blocks, c->stream);
    HIP_TRY(hipGetLastError());
    c->cov_valid = true;
    c->cov_rendered_grid = d.grid;
    return RTPBR_OK;
}

// The weights plane k and the frame's largest 1 - a from the coverage plane; the resolved count starts at 0 (the list's length stays)
static int cover_weights_enqueue(rtpbr_ctx* c, const rtpbr_coverage_params& d) {
    if (int r = frame_need(c, {ROW_cov_k, ROW_cov_linear})) return r;
    HIP_TRY(hipMemsetAsync(c->cov_list + 1, 0, 2 * sizeof(uint32_t), c->stream));
    launch_cover_weights(coverage_args(c, d), c->stream);
    return RTPBR_OK;
}

// The resolve and the tone map of every pixel: RTPBR_BUF_DENOISED_PIXELS from the linear colour in cov_linear.  live: the byte plane a
// filling last level wrote ("has a colour"), or nullptr ("has samples")
static void cover_resolve_enqueue(rtpbr_ctx* c, const rtpbr_coverage_params& d, const uint8_t* live) {
    ResolveArgs R{};
    R.cfg = c->cfg;
    R.image_buffer = c->image_buffer;
    R.linear = c->cov_linear;
    R.object = c->feat_object;
    R.coverage = c->coverage;
    R.k = c->cov_k;
    R.head = c->cov_list;
    R.out = c->denoised;
    R.width = c->cfg.width;
    R.height = c->cfg.height;
    R.resolve = d.resolve;
    R.live = live;
    launch_cover_resolve(R, c->stream);
}

extern "C" int rtpbr_render_coverage(rtpbr_ctx* c, const rtpbr_coverage_params* v) {
    if (!c) return fail(RTPBR_EINVAL, "null ctx");
    rtpbr_coverage_params d;
    if (int r = coverage_params(v, d)) return r;
    if (int r = whole_frame_state(c, FEATURE_TILES)) return r;
    return coverage_enqueue(c, d);
}

extern "C" int rtpbr_denoise_coverage(rtpbr_ctx* c, const rtpbr_denoise_params* p, const rtpbr_coverage_params* v, rtpbr_noise_stats* out) {
    if (!c) return fail(RTPBR_EINVAL, "null ctx");
    rtpbr_denoise_params d;
    rtpbr_coverage_params cv;
    float inv[4];
    if (int r = denoise_params(p, d, inv)) return r;
    if (int r = coverage_params(v, cv)) return r;
    if (int r = whole_frame_state(c, FEATURE_TILES)) return r;
    if (int r = coverage_enqueue(c, cv)) return r;
    if (int r = cover_weights_enqueue(c, cv)) return r;
    if (d.iterations == 0) {      // rtpbr_denoise's tone-map-only pass
        if (int r = denoise_levels(c, 0, d.demodulate, inv, FilterChain{})) return r;
    } else {
        if (int r = denoised_alloc(c, d.iterations)) return r;
        // option coverage_fill: the filling levels and the resolve that asks them who has a colour (not read with iterations = 0: no
        // level, nothing is filled, the counters keep the last filling call's)
        const bool fill = c->coverage_fill != 0;
        if (fill)
            if (int r = frame_need(c, {ROW_cov_live})) return r;
        FilterChain ch;
        ch.form = ATROUS_LINEAR | (fill ? ATROUS_FILL : 0u);
        ch.cover_k = c->cov_k;
        if (int r = denoise_levels(c, d.iterations, d.demodulate, inv, ch.on(c->image_buffer, c->cov_linear))) return r;
        cover_resolve_enqueue(c, cv, fill ? c->cov_live : nullptr);
    }
    HIP_TRY(hipGetLastError());
    if (!out) return RTPBR_OK;
    uint32_t head[COVER_HEAD];
    HIP_TRY(hipMemcpyAsync(head, c->cov_list, sizeof head, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    out->pixels_estimated = head[1];
    out->pixels_above = head[0];
    memcpy(&out->max_noise, &head[2], sizeof(float));
    return RTPBR_OK;
}

extern "C" int rtpbr_read_coverage(rtpbr_ctx* c, void* dst, size_t nbytes) {
    if (!c || !c->have_cfg) return fail(RTPBR_ESTATE, "set_config first");
    if (!c->coverage) return fail(RTPBR_ESTATE, "no coverage yet: call rtpbr_render_coverage / rtpbr_denoise_coverage first");
    if (!dst || nbytes != (size_t)c->cfg.width * c->cfg.height * sizeof(int4)) return fail(RTPBR_EINVAL, "destination size does not match the coverage plane");
    if (int r = set_dev(c)) return r;
    HIP_TRY(hipMemcpyAsync(dst, c->coverage, nbytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RTPBR_OK;
}

// ---- temporal reuse (rt_reproject.hip): rtpbr_set_camera + rtpbr_refresh that keeps what the new view can reuse

// p == NULL: the defaults; RTPBR_EINVAL for a parameter out of range
static int reproject_params(const rtpbr_reproject_params* p, rtpbr_reproject_params& d) {
    if (p) {
        d = *p;
    } else {
        d.max_history = RTPBR_REPROJECT_DEFAULT_MAX_HISTORY;
        d.depth_tolerance = RTPBR_REPROJECT_DEFAULT_DEPTH_TOLERANCE;
        d.normal_cos = RTPBR_REPROJECT_DEFAULT_NORMAL_COS;
    }
    if (!(d.max_history > 0.0f) || !std::isfinite(d.max_history)) return fail(RTPBR_EINVAL, "reproject max_history must be finite and > 0");
    if (!(d.depth_tolerance >= 0.0f) || !std::isfinite(d.depth_tolerance)) return fail(RTPBR_EINVAL, "reproject depth_tolerance must be finite and >= 0");
    if (!(d.normal_cos >= -1.0f && d.normal_cos <= 1.0f)) return fail(RTPBR_EINVAL, "reproject normal_cos must be within -1..1");
    return RTPBR_OK;
}

// the states rtpbr_reproject and rtpbr_reproject_scene refuse (`who`: the call's name)
static int reproject_state(rtpbr_ctx* c, const char* who) {
    if (int r = whole_frame_state(c, "%s works on the whole frame: not with tiles of world > 1", who)) return r;
    if (!c->history_ok)
        return fail(RTPBR_ESTATE, "%s: set_config / set_scene / set_shape_data / set_env ran since the last refresh or reproject: "
                                  "image_buffer is no history of this scene (call rtpbr_refresh)", who);
    return RTPBR_OK;
}

// Steps 1..8 of rtpbr_reproject (include/rtpbr.h) after every refusal has been ruled out.  objs != nullptr (rtpbr_reproject_scene):
// step 5 applies the new object table first, `table` (host, n * SCENE_MOTION_WORDS floats) is what the scene kernel reads and
// cam may be nullptr (the camera stays).
static int reproject_run(rtpbr_ctx* c, const rtpbr_camera* cam, const rtpbr_reproject_params& d, const rtpbr_object* objs = nullptr, int n_objs = 0,
                         int scale10 = 0, const float* table = nullptr) {
    if (int r = set_dev(c)) return r;
    if (int r = flush_shade(c)) return r;
    if (int r = rt_order_after_reads(c, W_IMAGE_BUFFER | W_RAY_BUFFER | W_DIFF_BUFFER | W_DIFF_PIXELS)) return r;
    if (!c->feat_valid)
        if (int r = rtpbr_render_features(c)) return r;      // the features of the old camera (and the old scene)
    const size_t n = (size_t)c->cfg.width * c->cfg.height;
    if (int r = frame_need(c, {ROW_hist_image, ROW_hist_guides, ROW_hist_object, ROW_motion})) return r;
    if (objs)
        if (int r = frame_need(c, {ROW_scene_motion})) return r;
    if (c->noise_moments) {      // the moments move with the image
        if (int r = frame_need(c, {ROW_hist_moments})) return r;
        if (int r = rt_order_after_reads(c, W_MOMENTS)) return r;
        HIP_TRY(hipMemcpyAsync(c->hist_moments, c->noise_moments, n * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
    }
    const bool warp_half = c->half_mode.warp != 0 && c->half_a != nullptr;      // rtpbr_set_half_mode: half A moves with the image
    if (warp_half) {
        if (int r = frame_need(c, {ROW_hist_half})) return r;
        if (int r = rt_order_after_reads(c, W_HALF)) return r;
        HIP_TRY(hipMemcpyAsync(c->hist_half, c->half_a, n * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
    }
    const CamFrame old_frame = c->P.cam;
    // copies, not pointer swaps: the public buffers keep the addresses rtpbr_buffer_device_ptr handed out
    HIP_TRY(hipMemcpyAsync(c->hist_image, c->image_buffer, n * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->hist_guides, c->feat_guides, n * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->hist_object, c->feat_object, n * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
    if (objs) {
        // (rtpbr_set_scene synchronises the stream after its own upload: the caller's `table` has been read by then)
        HIP_TRY(hipMemcpyAsync(c->scene_motion, table, sizeof(float) * (size_t)n_objs * SCENE_MOTION_WORDS, hipMemcpyHostToDevice, c->stream));
        if (int r = rtpbr_set_scene(c, objs, n_objs, scale10)) return r;
    }
    if (cam)
        if (int r = rtpbr_set_camera(c, cam)) return r;
    if (int r = rtpbr_render_features(c)) return r;          // the features of the new camera (feat_valid from here on)
    if (int r = rt_order_after_reads(c, W_MOTION)) return r;
    ReprojArgs A;
    A.cam0 = old_frame;
    A.cam1 = c->P.cam;
    A.cam1.inv_w = 1.0f / (float)c->cfg.width;
    A.cam1.inv_h = 1.0f / (float)c->cfg.height;
    A.hist_image = c->hist_image;
    A.hist_nz = c->hist_guides;
    A.hist_object = c->hist_object;
    A.new_nz = c->feat_guides;
    A.new_object = c->feat_object;
    A.image_buffer = c->image_buffer;
    A.motion = c->motion;
    A.ray_buffer = c->ray_buffer;
    A.diff_buffer = c->diff_buffer;
    A.diff_pixels = c->diff_pixels;
    A.max_history = d.max_history;
    A.depth_tol = d.depth_tolerance;
    A.normal_cos = d.normal_cos;
    A.width = c->cfg.width;
    A.height = c->cfg.height;
    A.pinhole = c->cfg.camera_kind == RTPBR_CAMERA_PINHOLE;
    A.adaptive = c->cfg.adaptive_sampling;
    A.normal_local = c->cfg.normal_space == RTPBR_NORMAL_LOCAL;
    A.hist_moments = c->noise_moments ? c->hist_moments : nullptr;
    A.moments = c->noise_moments;
    A.snapshot = c->noise_snapshot;
    A.hist_half = warp_half ? c->hist_half : nullptr;
    A.half_a = c->half_a;
    if (objs) launch_reproject_scene(A, c->scene_motion, n_objs, c->stream);
    else launch_reproject(A, c->stream);
    HIP_TRY(hipGetLastError());
    // the warped history is one body of samples: it lies in B — unless half A came along (the gather wrote it); sh = the warped image
    if (int r = half_restart(c, true, warp_half)) return r;
    c->history_ok = true;
    return RTPBR_OK;
}

extern "C" int rtpbr_reproject(rtpbr_ctx* c, const rtpbr_camera* cam, const rtpbr_reproject_params* p) {
    if (!c || !cam) return fail(RTPBR_EINVAL, "null argument");
    rtpbr_reproject_params d;
    if (int r = reproject_params(p, d)) return r;
    // every refusal before anything changes
    if (int r = reproject_state(c, "rtpbr_reproject")) return r;
    return reproject_run(c, cam, d);
}

// rtpbr_reproject for a scene whose objects moved rigidly (include/rtpbr.h): the new table must be the current one up to
// positions and rotations; the old and new positions and matrices go to the scene kernel (rt_reproject.hip).
extern "C" int rtpbr_reproject_scene(rtpbr_ctx* c, const rtpbr_camera* cam, const rtpbr_object* objs, int n, int scale10,
                                     const rtpbr_reproject_params* p) {
    if (!c || !objs) return fail(RTPBR_EINVAL, "null argument");
    rtpbr_reproject_params d;
    if (int r = reproject_params(p, d)) return r;
    if (int r = reproject_state(c, "rtpbr_reproject_scene")) return r;
    static const char* const NOT_RIGID = "not a rigid motion: use rtpbr_set_scene + rtpbr_refresh";
    if (n != c->n_obj) return fail(RTPBR_EINVAL, NOT_RIGID);
    float table[MAX_OBJ * SCENE_MOTION_WORDS];
    for (int i = 0; i < n; i++) {
        const rtpbr_object& o0 = c->obj[i];
        const rtpbr_object o1 = stored_object(objs[i], scale10);
        const rtpbr_transform &t0 = o0.transform, &t1 = o1.transform;
        if (o1.type != o0.type || memcmp(t1.scale, t0.scale, sizeof t0.scale) || memcmp(&o1.material, &o0.material, sizeof o0.material))
            return fail(RTPBR_EINVAL, NOT_RIGID);
        float* t = table + i * SCENE_MOTION_WORDS;
        const bool moved = memcmp(t1.position, t0.position, sizeof t0.position) || memcmp(t1.matrix, t0.matrix, sizeof t0.matrix);
        t[0] = moved ? 1.0f : 0.0f;
        memcpy(t + 1, t0.position, 12);
        memcpy(t + 4, t1.position, 12);
        memcpy(t + 7, t0.matrix, 36);
        memcpy(t + 16, t1.matrix, 36);
    }
    return reproject_run(c, cam, d, objs, n, scale10, table);
}

// ---- noise estimation and the variance-guided a-trous (rt_noise.hip)
static const char* const NOISE_TILES = "rtpbr_noise_update / rtpbr_noise_estimate / rtpbr_denoise_guided work on the whole frame: not with tiles of world > 1";

extern "C" int rtpbr_noise_update(rtpbr_ctx* c) {
    if (!c) return fail(RTPBR_EINVAL, "null ctx");
    if (!c->have_cfg) return fail(RTPBR_ESTATE, "set_config first");
    if (c->world > 1) return fail(RTPBR_ESTATE, NOISE_TILES);
    if (int r = set_dev(c)) return r;
    if (int r = flush_shade(c)) return r;
    if (int r = frame_need(c, {ROW_noise_moments, ROW_noise_snapshot})) return r;
    if (int r = rt_order_after_reads(c, W_MOMENTS)) return r;
    NoiseArgs A{};
    A.image_buffer = c->image_buffer;
    A.snapshot = c->noise_snapshot;
    A.moments = c->noise_moments;
    A.width = c->cfg.width;
    A.height = c->cfg.height;
    launch_noise_update(A, c->stream);
    HIP_TRY(hipGetLastError());
    return RTPBR_OK;
}

extern "C" int rtpbr_set_noise_tracking(rtpbr_ctx* c, int mode) {
    if (!c) return fail(RTPBR_EINVAL, "null ctx");
    if (mode != RTPBR_NOISE_TRACK_OFF && mode != RTPBR_NOISE_TRACK_SAMPLES)
        return fail(RTPBR_EINVAL, "rtpbr_set_noise_tracking: mode must be RTPBR_NOISE_TRACK_OFF or RTPBR_NOISE_TRACK_SAMPLES");
    if (mode == RTPBR_NOISE_TRACK_SAMPLES)      // everything deposited so far is one batch; the samples to come are batches of one
        if (int r = rtpbr_noise_update(c)) return r;
    c->noise_tracking = mode;
    return RTPBR_OK;
}

// the statistics' shards, zeroed on the stream for the kernel that is enqueued next (noise_stats_read brings them back)
static int noise_stats_zero(rtpbr_ctx* c) {
    if (!c->noise_stats) HIP_TRY(hipMalloc(&c->noise_stats, NOISE_SHARDS * sizeof(NoiseStats)));
    HIP_TRY(hipMemsetAsync(c->noise_stats, 0, NOISE_SHARDS * sizeof(NoiseStats), c->stream));
    return RTPBR_OK;
}

// the estimate pass on the stream (no read-back): RTPBR_BUF_NOISE, the guided filter's level-0 variance and the statistics
static int noise_estimate_enqueue(rtpbr_ctx* c, float threshold) {
    if (!c->feat_valid)
        if (int r = rtpbr_render_features(c)) return r;
    if (int r = set_dev(c)) return r;
    if (int r = flush_shade(c)) return r;
    if (int r = frame_need(c, {ROW_noise_moments, ROW_noise_snapshot, ROW_noise_map, ROW_noise_var})) return r;
    if (int r = rt_order_after_reads(c, W_NOISE)) return r;
    if (int r = noise_stats_zero(c)) return r;
    NoiseArgs A{};
    A.image_buffer = c->image_buffer;
    A.moments = c->noise_moments;
    A.object = c->feat_object;
    A.noise = c->noise_map;
    A.var0 = c->noise_var;
    A.stats = c->noise_stats;
    A.threshold = threshold;
    A.width = c->cfg.width;
    A.height = c->cfg.height;
    A.pool_batches = c->noise_estimator.pool_batches;
    A.pool_radius = c->noise_estimator.pool_radius;
    launch_noise_estimate(A, c->stream);
    HIP_TRY(hipGetLastError());
    return RTPBR_OK;
}

extern "C" int rtpbr_set_noise_estimator(rtpbr_ctx* c, const rtpbr_noise_estimator* e) {
    if (!c) return fail(RTPBR_EINVAL, "null ctx");
    static_assert(sizeof(rtpbr_noise_estimator) == 12, "three 4-byte members");
    rtpbr_noise_estimator d{RTPBR_NOISE_ESTIMATOR_DEFAULT_POOL_BATCHES, RTPBR_NOISE_ESTIMATOR_DEFAULT_POOL_RADIUS,
                            RTPBR_NOISE_ESTIMATOR_DEFAULT_MIN_SAMPLES};
    if (e) d = *e;
    if (d.pool_batches != 0 && (d.pool_batches < 3 || d.pool_batches > 64)) return fail(RTPBR_EINVAL, "noise estimator: pool_batches must be 0 or 3..64");
    if (d.pool_radius < 1 || d.pool_radius > 3) return fail(RTPBR_EINVAL, "noise estimator: pool_radius must be 1..3");
    if (d.min_samples < 0 || d.min_samples > 16777216) return fail(RTPBR_EINVAL, "noise estimator: min_samples must be 0..16777216");
    c->noise_estimator = d;
    return RTPBR_OK;
}

extern "C" int rtpbr_noise_estimate(rtpbr_ctx* c, float threshold, rtpbr_noise_stats* out) {
    if (!c) return fail(RTPBR_EINVAL, "null ctx");
    if (!(threshold >= 0.0f)) return fail(RTPBR_EINVAL, "noise threshold must be >= 0");
    if (int r = whole_frame_state(c, NOISE_TILES)) return r;
    if (int r = noise_estimate_enqueue(c, threshold)) return r;
    return noise_stats_read(c, out);
}

// the statistics a kernel left in noise_stats come back and are folded (blocks)
static int noise_stats_read(rtpbr_ctx* c, rtpbr_noise_stats* out) {
    static_assert(sizeof(NoiseStats) == 128, "one line per shard");
    std::vector<NoiseStats> sh(NOISE_SHARDS);
    HIP_TRY(hipMemcpyAsync(sh.data(), c->noise_stats, NOISE_SHARDS * sizeof(NoiseStats), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (out) {
        uint32_t est = 0, above = 0, mx = 0;
        for (const NoiseStats& s : sh) {
            est += s.estimated;
            above += s.above;
            mx = s.max_bits > mx ? s.max_bits : mx;
        }
        out->pixels_estimated = est;
        out->pixels_above = above;
        memcpy(&out->max_noise, &mx, sizeof(float));
    }
    return RTPBR_OK;
}

// ---- adaptive sampling of the complete-path form (rt_select.hip): select pixels, trace only those
static const char* const SELECT_TILES = "rtpbr_select_mask / rtpbr_select_noisy / rtpbr_sample_selected work on the whole frame: not with tiles of world > 1";

// ... with option select_tiers = T > 1 (A is filled, the selection's state cleared): the tiered passes, then the T cumulative counts
// come back (4 T bytes) and stay on the context — rtpbr_sample_selected and the counters "select_tier*" read them there
static int selection_build_tiered(rtpbr_ctx* c, const SelectArgs& A, int rule, int T, uint32_t* n_selected) {
    if (!c->sel_blocks_tiered) {
        // the first tiered selection of this frame size: sel_blocks gets the room of 8 tiers (nothing of the old one is kept)
        HIP_TRY(hipStreamSynchronize(c->stream));
        (void)hipFree(c->sel_blocks);
        c->sel_blocks = nullptr;
        c->sel_blocks_tiered = true;
        if (int r = frame_need(c, {ROW_sel_blocks})) {
            c->sel_blocks_tiered = false;
            return r;
        }
    }
    SelectTierArgs S{};
    S.A = A;
    S.A.blocks = c->sel_blocks;
    S.tiers = T;
    for (int k = 1; k < T; k++) S.bound[k - 1] = (float)((c->select_batch >> k) > 1 ? c->select_batch >> k : 1);
    launch_select_tiered(S, rule, c->stream);
    HIP_TRY(hipGetLastError());
    uint32_t cum[SELECT_MAX_TIERS] = {};
    const uint32_t nb = select_blocks(c->cfg.width, c->cfg.height);
    HIP_TRY(hipMemcpyAsync(cum, c->sel_blocks + (size_t)T * nb + 1, (size_t)T * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int t = 0; t < T; t++) c->sel_cum[t] = cum[t];
    c->sel_tiers = T;
    c->sel_count = cum[T - 1];
    c->have_selection = true;
    *n_selected = cum[T - 1];
    return RTPBR_OK;
}

// mark, scan, scatter on the stream, then the list's length (4 bytes) comes back: blocks
static int selection_build(rtpbr_ctx* c, SelectArgs& A, int rule, uint32_t* n_selected) {
    A.mask = c->sel_mask;
    A.blocks = c->sel_blocks;
    A.list = c->sel_list;
    A.width = c->cfg.width;
    A.height = c->cfg.height;
    c->have_selection = false;      // (until the new list's length is known)
    c->sel_count = 0;
    c->sel_tiers = 1;
    for (uint32_t& l : c->sel_cum) l = 0;
    const int T = c->select_tiers;
    if (T > 1) return selection_build_tiered(c, A, rule, T, n_selected);
    launch_select(A, rule, c->stream);
    HIP_TRY(hipGetLastError());
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, c->sel_blocks + select_blocks(c->cfg.width, c->cfg.height), sizeof total, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->sel_count = total;
    c->sel_cum[0] = total;
    c->have_selection = true;
    *n_selected = total;
    return RTPBR_OK;
}

extern "C" int rtpbr_select_mask(rtpbr_ctx* c, const uint8_t* mask, size_t nbytes, uint32_t* n_selected) {
    if (!c || !mask || !n_selected) return fail(RTPBR_EINVAL, "null argument");
    // (not whole_frame_state: a mask needs no shape data, and this call has never asked for it)
    if (!c->have_cfg || !c->have_scene || !c->have_cam) return fail(RTPBR_ESTATE, "set_config, set_scene and set_camera first");
    if (c->world > 1) return fail(RTPBR_ESTATE, SELECT_TILES);
    if (nbytes != (size_t)c->cfg.width * c->cfg.height) return fail(RTPBR_EINVAL, "rtpbr_select_mask: the mask must hold width * height bytes");
    if (int r = set_dev(c)) return r;
    if (int r = frame_need(c, {ROW_sel_mask, ROW_sel_list, ROW_sel_blocks})) return r;
    if (int r = rt_order_after_reads(c, W_SELECTION)) return r;
    // the caller's bytes go straight into RTPBR_BUF_SELECTION; the mark pass makes them 0 / 1 in place
    HIP_TRY(hipMemcpyAsync(c->sel_mask, mask, nbytes, hipMemcpyHostToDevice, c->stream));
    SelectArgs A{};
    A.host_mask = c->sel_mask;
    return selection_build(c, A, SELECT_MASK, n_selected);
}

// Option "select_lattice" (include/rtpbr.h): the state rtpbr_select_mask leaves for the lattice's mask, from ONE kernel that writes
// the plane and the list (rt_select.hip select_lattice_build).  The count is known here, so nothing is copied either way and
// nothing waits: the call enqueues and returns.  rtpbr_select_mask's refusals, in its order, once the value is a lattice.
static int select_lattice_option(rtpbr_ctx* c, long long value) {
    if (value == 0) return RTPBR_OK;
    LatticeArgs A{};
    if (!lattice_decode(value, &A.l)) return fail(RTPBR_EINVAL, RTPBR_SELECT_LATTICE_REFUSAL);
    // (a context without a device has no frame to select in)
    if (!c->have_cfg || !c->have_scene || !c->have_cam || c->headless) return fail(RTPBR_ESTATE, "set_config, set_scene and set_camera first");
    if (c->world > 1) return fail(RTPBR_ESTATE, SELECT_TILES);
    if (int r = set_dev(c)) return r;
    if (int r = frame_need(c, {ROW_sel_mask, ROW_sel_list, ROW_sel_blocks})) return r;
    if (int r = rt_order_after_reads(c, W_SELECTION)) return r;
    lattice_count(&A.l, c->cfg.width, c->cfg.height);
    A.mask = c->sel_mask;
    A.list = c->sel_list;
    A.width = c->cfg.width;
    A.height = c->cfg.height;
    c->have_selection = false;
    c->sel_count = 0;
    c->sel_tiers = 1;
    for (uint32_t& l : c->sel_cum) l = 0;
    launch_select_lattice(A, c->stream);
    HIP_TRY(hipGetLastError());
    // every lattice pixel is in tier 0 (the mask's byte 1): with select_tiers = T the pixels of tiers 0 .. t are all of them
    const uint32_t n = A.l.nx * A.l.ny;
    c->sel_tiers = c->select_tiers;
    for (int t = 0; t < c->sel_tiers; t++) c->sel_cum[t] = n;
    c->sel_count = n;
    c->have_selection = true;
    return RTPBR_OK;
}

extern "C" int rtpbr_select_noisy(rtpbr_ctx* c, float threshold, int dilate, uint32_t* n_selected) {
    if (!c || !n_selected) return fail(RTPBR_EINVAL, "null argument");
    if (!(threshold >= 0.0f)) return fail(RTPBR_EINVAL, "noise threshold must be >= 0");
    if (dilate < 0 || dilate > 3) return fail(RTPBR_EINVAL, "rtpbr_select_noisy: dilate must be 0..3");
    if (int r = whole_frame_state(c, NOISE_TILES)) return r;
    if (int r = noise_estimate_enqueue(c, threshold)) return r;
    if (int r = frame_need(c, {ROW_sel_mask, ROW_sel_list, ROW_sel_blocks})) return r;
    if (int r = rt_order_after_reads(c, W_SELECTION)) return r;
    SelectArgs A{};
    A.image_buffer = c->image_buffer;
    A.noise = c->noise_map;
    A.threshold = threshold;
    A.dilate = dilate;
    A.min_samples = (float)c->noise_estimator.min_samples;
    return selection_build(c, A, SELECT_NOISY, n_selected);
}

extern "C" int rtpbr_sample_selected(rtpbr_ctx* c, int n) {
    if (!c) return fail(RTPBR_EINVAL, "null ctx");
    // (not whole_frame_state: n is checked between the two states, and missing shape data is sample_call's to refuse)
    if (!c->have_cfg || !c->have_scene || !c->have_cam) return fail(RTPBR_ESTATE, "set_config, set_scene and set_camera first");
    if (n < 0) return fail(RTPBR_EINVAL, "n must be >= 0");
    if (c->world > 1) return fail(RTPBR_ESTATE, SELECT_TILES);
    if (c->cfg.kernel_form != RTPBR_FORM_COMPLETE_PATH)
        return fail(RTPBR_ESTATE, "rtpbr_sample_selected: the complete-path form only (the persistent-ray form has cfg.adaptive_sampling)");
    if (c->precision) return fail(RTPBR_ESTATE, "rtpbr_sample_selected: not with option precision = 1 (the tolerance flavour has no selected instances)");
    if (!c->have_selection) return fail(RTPBR_ESTATE, "rtpbr_sample_selected: no selection yet (rtpbr_select_mask / rtpbr_select_noisy first)");
    if (int r = tracked_sample_check(c)) return r;
    return sample_call(c, n, true);
}

extern "C" int rtpbr_denoise_guided(rtpbr_ctx* c, const rtpbr_denoise_guided_params* p) {
    if (!c) return fail(RTPBR_EINVAL, "null ctx");
    rtpbr_denoise_guided_params d;
    if (p) {
        d = *p;
    } else {
        d.iterations = RTPBR_DENOISE_GUIDED_DEFAULT_ITERATIONS;
        d.demodulate = RTPBR_DENOISE_GUIDED_DEFAULT_DEMODULATE;
        d.sigma_color = RTPBR_DENOISE_GUIDED_DEFAULT_SIGMA_COLOR;
        d.sigma_normal = RTPBR_DENOISE_GUIDED_DEFAULT_SIGMA_NORMAL;
        d.sigma_depth = RTPBR_DENOISE_GUIDED_DEFAULT_SIGMA_DEPTH;
        d.variance_floor = RTPBR_DENOISE_GUIDED_DEFAULT_VARIANCE_FLOOR;
    }
    const float sig[3] = {d.sigma_color, d.sigma_normal, d.sigma_depth};
    float inv[3];
    if (int r = denoise_params_check(d.iterations, d.demodulate, sig, inv, 3)) return r;
    const float sc2 = d.sigma_color * d.sigma_color;
    if (!(d.variance_floor > 0.0f) || !std::isfinite(d.variance_floor) || !std::isfinite(1.0f / (sc2 * d.variance_floor)))
        return fail(RTPBR_EINVAL, "denoise variance_floor must be finite and > 0 (and 1/(sigma_color^2 variance_floor) must not overflow)");
    if (int r = whole_frame_state(c, NOISE_TILES)) return r;
    if (d.iterations > 0) {
        if (int r = noise_estimate_enqueue(c, 0.0f)) return r;
    } else if (!c->feat_valid) {
        if (int r = rtpbr_render_features(c)) return r;
    }
    FilterChain ch;
    ch.guided = &d;
    return denoise_levels(c, d.iterations, d.demodulate, inv, ch);
}

// ---- the two-half error estimate of the denoised frame (rt_half.hip)
static const char* const HALF_TILES = "rtpbr_half_update / rtpbr_denoise_error / rtpbr_denoise_blend / rtpbr_denoise_blend_levels / rtpbr_blend_error / rtpbr_blend_error_display / rtpbr_select_error / rtpbr_select_blend_error work on the whole frame: not with tiles of world > 1";

// What refresh, rtpbr_write_buffer(RTPBR_BUF_IMAGE_BUFFER) and the reprojections do once A exists (enqueues only): A = 0 and the
// snapshot = 0 (snapshot_image false: the image is being zeroed too) or = image_buffer as the stream has it by now.  keep_a: A has
// been written by the caller (a reprojection that carries it, rtpbr_set_half_mode): the snapshot alone.
static int half_restart(rtpbr_ctx* c, bool snapshot_image, bool keep_a) {
    if (!c->half_a) return RTPBR_OK;
    if (int r = rt_order_after_reads(c, W_HALF)) return r;
    const size_t bytes = (size_t)c->cfg.width * c->cfg.height * sizeof(float4);
    if (!keep_a) HIP_TRY(hipMemsetAsync(c->half_a, 0, bytes, c->stream));
    if (snapshot_image) HIP_TRY(hipMemcpyAsync(c->half_snapshot, c->image_buffer, bytes, hipMemcpyDeviceToDevice, c->stream));
    else HIP_TRY(hipMemsetAsync(c->half_snapshot, 0, bytes, c->stream));
    return RTPBR_OK;
}

extern "C" int rtpbr_half_update(rtpbr_ctx* c) {
    if (!c) return fail(RTPBR_EINVAL, "null ctx");
    if (!c->have_cfg) return fail(RTPBR_ESTATE, "set_config first");
    if (c->world > 1) return fail(RTPBR_ESTATE, HALF_TILES);
    if (int r = set_dev(c)) return r;
    if (int r = flush_shade(c)) return r;
    if (int r = frame_need(c, {ROW_half_a, ROW_half_snapshot})) return r;
    if (int r = rt_order_after_reads(c, W_HALF)) return r;
    HalfArgs A{};
    A.image_buffer = c->image_buffer;
    A.snapshot = c->half_snapshot;
    A.half_a = c->half_a;
    A.width = c->cfg.width;
    A.height = c->cfg.height;
    launch_half_update(A, c->stream);
    HIP_TRY(hipGetLastError());
    return RTPBR_OK;
}

extern "C" int rtpbr_set_half_mode(rtpbr_ctx* c, const rtpbr_half_mode* m) {
    if (!c) return fail(RTPBR_EINVAL, "null ctx");
    rtpbr_half_mode d{RTPBR_HALF_MODE_DEFAULT_PER_SAMPLE, RTPBR_HALF_MODE_DEFAULT_WARP};
    if (m) d = *m;
    if ((d.per_sample != 0 && d.per_sample != 1) || (d.warp != 0 && d.warp != 1))
        return fail(RTPBR_EINVAL, "rtpbr_set_half_mode: per_sample and warp must be 0 or 1");
    if (d.per_sample && !c->half_mode.per_sample)      // everything deposited so far is one batch; the samples to come are batches of one
        if (int r = rtpbr_half_update(c)) return r;
    c->half_mode = d;
    return RTPBR_OK;
}

// What rtpbr_denoise_error and the blend calls do between their parameter checks and their allocations: the states they refuse
// (no_half: the call's "no half buffer yet" message, `who` fills its %s), the device, the pending shade
static int half_call_begin(rtpbr_ctx* c, const char* no_half, const char* who) {
    if (int r = whole_frame_state(c, HALF_TILES)) return r;
    if (!c->half_a) return fail(RTPBR_ESTATE, no_half, who);
    if (int r = set_dev(c)) return r;
    return flush_shade(c);
}

// B = image_buffer - A into its own buffer, enqueued here
static int half_b_enqueue(rtpbr_ctx* c) {
    if (int r = frame_need(c, {ROW_half_b})) return r;
    HalfArgs S{};
    S.image_buffer = c->image_buffer;
    S.half_a = c->half_a;
    S.half_b = c->half_b;
    S.width = c->cfg.width;
    S.height = c->cfg.height;
    launch_half_subtract(S, c->stream);
    return RTPBR_OK;
}

// e (NULL: the defaults) -> b, after the parameter checks of the blend calls
static int blend_params(const rtpbr_blend_params* e, const char* who, rtpbr_blend_params& b) {
    b = rtpbr_blend_params{RTPBR_BLEND_DEFAULT_RADIUS, RTPBR_BLEND_DEFAULT_Z, RTPBR_BLEND_DEFAULT_MIN_HALF_SAMPLES};
    if (e) b = *e;
    if (b.radius < 1 || b.radius > 3) return fail(RTPBR_EINVAL, "%s: radius must be 1..3", who);
    if (!(b.z >= 0.0f) || !std::isfinite(b.z)) return fail(RTPBR_EINVAL, "%s: z must be finite and >= 0", who);
    if (b.min_half_samples < 1 || b.min_half_samples > 16777216) return fail(RTPBR_EINVAL, "%s: min_half_samples must be 1..16777216", who);
    return RTPBR_OK;
}

extern "C" int rtpbr_denoise_error(rtpbr_ctx* c, const rtpbr_denoise_params* p, const rtpbr_error_params* e, float threshold,
                                   rtpbr_noise_stats* out) {
    if (!c) return fail(RTPBR_EINVAL, "null ctx");
    rtpbr_denoise_params d;
    float inv[4];
    if (int r = denoise_params(p, d, inv)) return r;
    const int radius = e ? e->radius : RTPBR_ERROR_DEFAULT_RADIUS;
    if (radius < 1 || radius > 3) return fail(RTPBR_EINVAL, "rtpbr_denoise_error: radius must be 1..3");
    if (!(threshold >= 0.0f)) return fail(RTPBR_EINVAL, "error threshold must be >= 0");
    if (int r = half_call_begin(c, "%s: no half buffer yet (rtpbr_half_update first)", "rtpbr_denoise_error")) return r;
    if (int r = frame_need(c, {ROW_half_da, ROW_half_db, ROW_denoised_error})) return r;
    if (int r = denoise_scratch_need(c, d.iterations)) return r;
    if (int r = rt_order_after_reads(c, W_ERROR)) return r;
    if (!c->feat_valid)
        if (int r = rtpbr_render_features(c)) return r;
    if (int r = half_b_enqueue(c)) return r;
    // the same filter on either half: "has samples" is the half's own count
    const FilterChain ch{};
    if (int r = denoise_levels(c, d.iterations, d.demodulate, inv, ch.on(c->half_a, c->half_da))) return r;
    if (int r = denoise_levels(c, d.iterations, d.demodulate, inv, ch.on(c->half_b, c->half_db))) return r;
    if (int r = noise_stats_zero(c)) return r;
    ErrorArgs A{};
    A.da = c->half_da;
    A.db = c->half_db;
    A.half_a = c->half_a;
    A.half_b = c->half_b;
    A.object = c->feat_object;
    A.error = c->denoised_error;
    A.stats = c->noise_stats;
    A.threshold = threshold;
    A.width = c->cfg.width;
    A.height = c->cfg.height;
    A.radius = radius;
    launch_half_error(A, c->stream);
    HIP_TRY(hipGetLastError());
    return noise_stats_read(c, out);
}

// ---- the bias-aware blend of the denoised and the raw frame (half_blend<R>, rt_half.hip)
static const char* const BLEND_NO_HALF = "%s: no half buffer yet (rtpbr_half_update or a dealing rtpbr_sample first)";

extern "C" int rtpbr_denoise_blend(rtpbr_ctx* c, const rtpbr_denoise_params* p, const rtpbr_blend_params* e, rtpbr_noise_stats* out) {
    if (!c) return fail(RTPBR_EINVAL, "null ctx");
    rtpbr_denoise_params d;
    float inv[4];
    if (int r = denoise_params(p, d, inv)) return r;
    rtpbr_blend_params b;
    if (int r = blend_params(e, "rtpbr_denoise_blend", b)) return r;
    if (int r = half_call_begin(c, BLEND_NO_HALF, "rtpbr_denoise_blend")) return r;
    if (int r = frame_need(c, {ROW_half_da, ROW_half_db, ROW_half_fd, ROW_blend_weight})) return r;
    if (int r = denoised_alloc(c, d.iterations)) return r;      // (and behind reads of RTPBR_BUF_DENOISED_PIXELS)
    if (int r = rt_order_after_reads(c, W_BLEND)) return r;
    if (!c->feat_valid)
        if (int r = rtpbr_render_features(c)) return r;
    if (int r = half_b_enqueue(c)) return r;
    // three runs of the same filter, each stopping before the tone map
    FilterChain ch;
    ch.form = ATROUS_LINEAR;
    if (int r = denoise_levels(c, d.iterations, d.demodulate, inv, ch.on(c->image_buffer, c->half_fd))) return r;
    if (int r = denoise_levels(c, d.iterations, d.demodulate, inv, ch.on(c->half_a, c->half_da))) return r;
    if (int r = denoise_levels(c, d.iterations, d.demodulate, inv, ch.on(c->half_b, c->half_db))) return r;
    if (int r = noise_stats_zero(c)) return r;
    BlendArgs A{};
    A.cfg = c->cfg;
    A.image_buffer = c->image_buffer;
    A.half_a = c->half_a;
    A.half_b = c->half_b;
    A.fd = c->half_fd;
    A.fa = c->half_da;
    A.fb = c->half_db;
    A.object = c->feat_object;
    A.weight = c->blend_weight;
    A.out = c->denoised;
    A.stats = c->noise_stats;
    A.min_half = (float)b.min_half_samples;
    A.z2 = b.z * b.z;
    A.width = c->cfg.width;
    A.height = c->cfg.height;
    A.radius = b.radius;
    launch_half_blend(A, c->stream);
    HIP_TRY(hipGetLastError());
    return noise_stats_read(c, out);
}

// ---- the same blend across the a-trous levels (level_blend<R, FIRST, LAST>, rt_half.hip), and with `window` the error estimate of
// its frame (rtpbr_blend_error: the ERR instances and blend_error<R>; `display`, rtpbr_blend_error_display: the slope goes to a
// plane of its own and the DISPLAY instances read it per tap).
// Option blend_coverage = 1 with K > 0 (all three calls; with no level the option is not read): the three chains run atrous_level's
// COVER form on the one plane k of cover_weights, the running colour lives in cov_linear where the LIN last level leaves it
// linear, and cover_resolve makes RTPBR_BUF_DENOISED_PIXELS from it ("has a colour" = image_buffer's count > 0).  Weight, depth,
// both sets of statistics and the error plane are those of the colour before the resolve.  cov_k and cov_linear are rtpbr_denoise_coverage's planes: both calls run on the
// context's one stream and neither keeps them across calls.
// Option blend_fill = 1 with K > 0 (all three calls; with no level the option is not read and nothing is filled): the three chains
// run atrous_level's FILL form, with blend_coverage its COVER and FILL form, each filling its own empty pixels; image_buffer's chain
// counts into the call's shards, the halves' into the set nobody reads.  The last level is level_blend's FILL instance, which shows
// the pixels without samples from level K's record, counts them and (LIN) writes cov_live for cover_resolve's FILL form.
static int blend_levels(rtpbr_ctx* c, const char* who, const rtpbr_denoise_params* p, const rtpbr_blend_params* e,
                        const rtpbr_error_params* w, bool with_error, bool display, float threshold, rtpbr_noise_stats* out) {
    if (!c) return fail(RTPBR_EINVAL, "null ctx");
    rtpbr_denoise_params d;
    float inv[4];
    if (int r = denoise_params(p, d, inv)) return r;
    rtpbr_blend_params b;
    if (int r = blend_params(e, who, b)) return r;
    const int window = w ? w->radius : RTPBR_ERROR_DEFAULT_RADIUS;
    if (with_error) {
        if (window < 1 || window > 3) return fail(RTPBR_EINVAL, "%s: the window's radius must be 1..3", who);
        if (!(threshold >= 0.0f)) return fail(RTPBR_EINVAL, "error threshold must be >= 0");
    }
    if (int r = half_call_begin(c, BLEND_NO_HALF, who)) return r;
    const size_t n = (size_t)c->cfg.width * c->cfg.height;
    const int K = d.iterations;
    const bool cover = c->blend_coverage != 0 && K > 0;
    const bool fill = c->blend_fill != 0 && K > 0;
    const rtpbr_coverage_params cv{c->blend_coverage_grid, c->blend_coverage_power, c->blend_coverage_resolve};
    if (cover && ((long long)cv.grid * c->cfg.width > 65535 || (long long)cv.grid * c->cfg.height > 65535))
        return fail(RTPBR_EINVAL, "coverage: grid x resolution out of range (1..65535)");      // (coverage_enqueue's, before anything is allocated)
    if (int r = frame_need(c, {ROW_blend_weight, ROW_blend_depth, ROW_levels_scratch})) return r;
    if (with_error)
        if (int r = frame_need(c, {ROW_blend_error, ROW_blend_x})) return r;
    if (display)
        if (int r = frame_need(c, {ROW_blend_slope})) return r;
    if (int r = denoised_alloc(c, 0)) return r;      // (and behind reads of RTPBR_BUF_DENOISED_PIXELS)
    if (int r = rt_order_after_reads(c, W_BLEND | W_DEPTH | (with_error ? W_BLEND_ERROR : 0u))) return r;
    if (!c->feat_valid)
        if (int r = rtpbr_render_features(c)) return r;
    if (int r = half_b_enqueue(c)) return r;
    if (int r = noise_stats_zero(c)) return r;
    if (cover) {      // the plane (rendered when stale, at the option's grid), the weights and the resolved count at 0, as rtpbr_denoise_coverage
        if (int r = coverage_enqueue(c, cv)) return r;
        if (int r = cover_weights_enqueue(c, cv)) return r;
        if (!c->blend_resolved) HIP_TRY(hipMalloc(&c->blend_resolved, sizeof(uint32_t)));
        if (fill)
            if (int r = frame_need(c, {ROW_cov_live})) return r;
    }
    if (fill)
        if (int r = fill_counts_zero(c)) return r;
    LevelsArgs A{};
    if (with_error) {      // the ERR instances: XA and XB beside the frame, the slope into the error plane (display: into its own)
        A.xa = c->blend_x;
        A.xb = c->blend_x + n;
        A.slope = display ? c->blend_slope : c->blend_error;
    }
    A.cfg = c->cfg;
    A.image_buffer = c->image_buffer;
    A.half_a = c->half_a;
    A.half_b = c->half_b;
    A.albedo = c->feat_albedo;
    A.object = c->feat_object;
    A.weight = c->blend_weight;
    A.depth = c->blend_depth;
    A.out = c->denoised;
    A.stats = c->noise_stats;
    A.min_half = (float)b.min_half_samples;
    A.z2 = b.z * b.z;
    A.demodulate = d.demodulate;
    A.width = c->cfg.width;
    A.height = c->cfg.height;
    A.radius = b.radius;
    // the last level's FILL instance shows the pixels without samples, counts them and (LIN) writes cov_live for the resolve
    uint32_t* const counts = fill ? c->fill_counts : nullptr;
    uint8_t* const live = fill && cover ? c->cov_live : nullptr;
    const unsigned blend_form = cover ? BLEND_LIN : 0u;
    if (K == 0) {      // rtpbr_denoise's pass, weight 1, depth 0
        if (int r = denoise_levels(c, 0, d.demodulate, inv, FilterChain{})) return r;
        if (!launch_level_blend(A, LEVEL_ONLY | blend_form, c->stream, counts, live)) return no_instance("level_blend");
    }
    // the K levels of the three chains in lock step through the non-last instances: chain j keeps level k in plane 2 j + (k & 1),
    // so level k - 1 is still there when the window kernel compares the two
    DenoiseArgs F = denoise_args(c, d.demodulate, inv);
    if (cover) {
        F.cover_k = c->cov_k;      // k is geometric: one plane for the three chains
        A.out = c->cov_linear;     // the running colour and, after the LIN last level, what the resolve reads
    }
    const unsigned chain_form = (cover ? ATROUS_COVER : 0u) | (fill ? ATROUS_FILL : 0u);
    const float4* const chain_in[3] = {c->image_buffer, c->half_a, c->half_b};
    for (int k = 0; k < K; k++) {      // k + 1 is the level's number in include/rtpbr.h
        const unsigned position = level_position(k, K), kept = position & LEVEL_FIRST;      // (a chain keeps every level's record: none is its last)
        float4* now[3];
        const float4* before[3];
        for (int j = 0; j < 3; j++) {
            F.image_buffer = chain_in[j];
            level_args(F, k, kept, inv, c->levels_scratch + (size_t)(2 * j) * n, nullptr, n);
            now[j] = F.dst;
            before[j] = F.src;
            if (fill) F.fill = c->fill_counts + (j == 0 ? 0 : FILL_COUNT_WORDS);      // (shares vsrc's word: the plain filter)
            if (!launch_atrous_level(F, kept | chain_form, c->stream)) return no_instance("atrous_level");
        }
        A.kd = now[0];
        A.ka = now[1];
        A.kb = now[2];
        A.pd = before[0];
        A.pa = before[1];
        A.pb = before[2];
        if (!launch_level_blend(A, position | blend_form, c->stream, counts, live)) return no_instance("level_blend");
    }
    if (cover) {      // the resolve and the tone map of every pixel, from the blended linear colour
        cover_resolve_enqueue(c, cv, live);      // option blend_fill: "has a colour" is what the LIN last level wrote
        HIP_TRY(hipMemcpyAsync(c->blend_resolved, c->cov_list + 1, sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
    }
    HIP_TRY(hipGetLastError());
    if (!with_error) return noise_stats_read(c, out);
    // the statistics are the error plane's: the blend's own are not handed out by this call
    if (int r = noise_stats_zero(c)) return r;
    BlendErrorArgs E{};
    E.lx = c->blend_x;
    E.half_a = c->half_a;
    E.half_b = c->half_b;
    E.object = c->feat_object;
    E.error = c->blend_error;
    E.slope = display ? c->blend_slope : nullptr;
    E.stats = c->noise_stats;
    E.threshold = threshold;
    E.min_half = (float)b.min_half_samples;
    E.width = c->cfg.width;
    E.height = c->cfg.height;
    E.radius = window;
    launch_blend_error(E, c->stream);
    HIP_TRY(hipGetLastError());
    return noise_stats_read(c, out);
}

extern "C" int rtpbr_denoise_blend_levels(rtpbr_ctx* c, const rtpbr_denoise_params* p, const rtpbr_blend_params* e, rtpbr_noise_stats* out) {
    return blend_levels(c, "rtpbr_denoise_blend_levels", p, e, nullptr, false, false, 0.0f, out);
}

extern "C" int rtpbr_blend_error(rtpbr_ctx* c, const rtpbr_denoise_params* p, const rtpbr_blend_params* e, const rtpbr_error_params* w,
                                 float threshold, rtpbr_noise_stats* out) {
    return blend_levels(c, "rtpbr_blend_error", p, e, w, true, false, threshold, out);
}

extern "C" int rtpbr_blend_error_display(rtpbr_ctx* c, const rtpbr_denoise_params* p, const rtpbr_blend_params* e,
                                         const rtpbr_error_params* w, float threshold, rtpbr_noise_stats* out) {
    return blend_levels(c, "rtpbr_blend_error_display", p, e, w, true, true, threshold, out);
}

// The selection by an error estimate: `plane` is the estimate's, `who` the call (it fills the %s of its messages), no_estimate
// what it says while the plane has not been made
static int select_by_error(rtpbr_ctx* c, float* rtpbr_ctx::*plane, const char* who, const char* no_estimate, float threshold, int dilate,
                           uint32_t* n_selected) {
    if (!c || !n_selected) return fail(RTPBR_EINVAL, "null argument");
    if (!(threshold >= 0.0f)) return fail(RTPBR_EINVAL, "error threshold must be >= 0");
    if (dilate < 0 || dilate > 3) return fail(RTPBR_EINVAL, "%s: dilate must be 0..3", who);
    if (int r = whole_frame_state(c, HALF_TILES)) return r;
    if (!(c->*plane) || !c->half_a) return fail(RTPBR_ESTATE, no_estimate, who);
    if (int r = set_dev(c)) return r;
    if (int r = flush_shade(c)) return r;
    if (int r = frame_need(c, {ROW_sel_mask, ROW_sel_list, ROW_sel_blocks})) return r;
    if (int r = rt_order_after_reads(c, W_SELECTION)) return r;
    SelectArgs A{};
    A.image_buffer = c->image_buffer;
    A.noise = c->*plane;
    A.half_a = c->half_a;
    A.threshold = threshold;
    A.dilate = dilate;
    A.min_samples = (float)c->noise_estimator.min_samples;
    return selection_build(c, A, SELECT_ERROR, n_selected);
}

extern "C" int rtpbr_select_error(rtpbr_ctx* c, float threshold, int dilate, uint32_t* n_selected) {
    return select_by_error(c, &rtpbr_ctx::denoised_error, "rtpbr_select_error", "%s: no error estimate yet (rtpbr_denoise_error first)", threshold,
                           dilate, n_selected);
}

// rtpbr_select_error's rule and kernels on RTPBR_BUF_BLEND_ERROR
extern "C" int rtpbr_select_blend_error(rtpbr_ctx* c, float threshold, int dilate, uint32_t* n_selected) {
    return select_by_error(c, &rtpbr_ctx::blend_error, "rtpbr_select_blend_error", "%s: no error estimate yet (rtpbr_blend_error first)", threshold,
                           dilate, n_selected);
}

// ---- the present stage (rt_present.hip): a display buffer -> the packed 8-bit top-down frame, on the device
extern "C" int rtpbr_present(rtpbr_ctx* c, const rtpbr_present_params* p) {
    if (!c) return fail(RTPBR_EINVAL, "null ctx");
    rtpbr_present_params d;
    if (p) {
        d = *p;
    } else {
        d.source = RTPBR_PRESENT_DEFAULT_SOURCE;
        d.format = RTPBR_PRESENT_DEFAULT_FORMAT;
        d.dither = RTPBR_PRESENT_DEFAULT_DITHER;
    }
    if (d.source < RTPBR_PRESENT_PIXELS || d.source > RTPBR_PRESENT_ACCUM) return fail(RTPBR_EINVAL, "present source must be RTPBR_PRESENT_PIXELS, _DENOISED or _ACCUM");
    if (d.format != RTPBR_PRESENT_RGB8 && d.format != RTPBR_PRESENT_RGBA8) return fail(RTPBR_EINVAL, "present format must be RTPBR_PRESENT_RGB8 or _RGBA8");
    if (d.dither != 0 && d.dither != 1) return fail(RTPBR_EINVAL, "present dither must be 0 or 1");
    if (!c->have_cfg || c->headless) return fail(RTPBR_ESTATE, "set_config first");
    if (d.source == RTPBR_PRESENT_DENOISED && !c->denoised) return fail(RTPBR_ESTATE, "rtpbr_present: no denoised image yet (rtpbr_denoise / rtpbr_denoise_guided first)");
    if (int r = set_dev(c)) return r;
    if (int r = frame_need(c, {ROW_present})) return r;
    if (int r = rt_order_after_reads(c, W_PRESENT)) return r;
    PresentArgs A{};
    A.cfg = c->cfg;
    A.src3 = d.source == RTPBR_PRESENT_DENOISED ? c->denoised : c->image_pixels;
    A.src4 = c->image_buffer;
    A.out = c->present;
    A.width = c->cfg.width;
    A.height = c->cfg.height;
    launch_present(A, d.source == RTPBR_PRESENT_ACCUM, d.format == RTPBR_PRESENT_RGBA8, d.dither != 0, c->stream);
    HIP_TRY(hipGetLastError());
    c->present_channels = d.format == RTPBR_PRESENT_RGBA8 ? 4 : 3;
    return RTPBR_OK;
}

extern "C" int rtpbr_sync(rtpbr_ctx* c) {
    if (!c) return fail(RTPBR_EINVAL, "null ctx");
    if (int r = set_dev(c)) return r;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->copy_stream) HIP_TRY(hipStreamSynchronize(c->copy_stream));      // asynchronous read-backs have landed too
    // a gather enqueued earlier has run by now: what did the communicator make of it (any rank)?
    return rt_rccl_check_async(c);
}

static int buf_ptr(rtpbr_ctx* c, int which, void** p, size_t* n) {
    if (!c || !c->have_cfg) return fail(RTPBR_ESTATE, "set_config first");
    const size_t np = (size_t)c->cfg.width * c->cfg.height;
    constexpr bool reported = true;
    unsigned group = 0;
#define X(m, T, bytes, g, zeroed, id, writable) \
    if (id != FRAME_PRIVATE && which == id) {   \
        *p = c->m;                              \
        *n = bytes;                             \
        group = g;                              \
    }
    RT_FRAME_BUFFERS(X)
#undef X
    if (!group) return fail(RTPBR_EINVAL, "unknown buffer id");
    // (the core buffers came with the configuration; the others exist from the call named in their row on)
    if (group != FRAME_CORE && !*p) return fail(RTPBR_ESTATE, "buffer not allocated yet: call rtpbr_render_features / rtpbr_denoise / rtpbr_reproject / rtpbr_noise_* / rtpbr_select_* / rtpbr_present / rtpbr_half_update / rtpbr_denoise_error / rtpbr_denoise_blend / rtpbr_denoise_blend_levels / rtpbr_blend_error first");
    return 0;
}

extern "C" int rtpbr_read_buffer(rtpbr_ctx* c, int which, void* dst, size_t nbytes) {
    void* p;
    size_t n;
    if (int r = buf_ptr(c, which, &p, &n)) return r;
    if (!dst || nbytes != n) return fail(RTPBR_EINVAL, "destination size does not match the buffer");
    if (int r = set_dev(c)) return r;
    if (which == RTPBR_BUF_RAY_BUFFER)
        if (int r = flush_shade(c)) return r;
    HIP_TRY(hipMemcpyAsync(dst, p, n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RTPBR_OK;
}

// canvas.set_image(image_pixels), src/main.py:64: the consumer takes the frame where it is
extern "C" int rtpbr_buffer_device_ptr(rtpbr_ctx* c, int which, void** device_ptr, size_t* nbytes) {
    void* p;
    size_t n;
    if (int r = buf_ptr(c, which, &p, &n)) return r;
    if (!device_ptr) return fail(RTPBR_EINVAL, "rtpbr_buffer_device_ptr: result pointer is required");
    if (which == RTPBR_BUF_RAY_BUFFER) {      // its holder reads ray_buffer unannounced: shade now, and with every launch from here on
        if (int r = flush_shade(c)) return r;
        c->ray_ptr_out = true;
    }
    *device_ptr = p;
    if (nbytes) *nbytes = n;
    return RTPBR_OK;
}

extern "C" int rtpbr_read_buffer_async(rtpbr_ctx* c, int which, void* dst, size_t nbytes, int* ticket) {
    void* p;
    size_t n;
    if (int r = buf_ptr(c, which, &p, &n)) return r;
    if (which == RTPBR_BUF_RAY_BUFFER)
        if (int r = flush_shade(c)) return r;
    if (!dst || !ticket || nbytes != n) return fail(RTPBR_EINVAL, "rtpbr_read_buffer_async: destination, ticket and the buffer's exact size are required");
    bool pinned = false;
    for (size_t i = 0; i < c->host_blocks.size() && !pinned; i++) {
        const char* b = (const char*)c->host_blocks[i];
        pinned = (const char*)dst >= b && (const char*)dst + n <= b + c->host_sizes[i];
    }
    if (!pinned) return fail(RTPBR_EINVAL, "rtpbr_read_buffer_async: the destination must lie inside a block of rtpbr_host_alloc (page-locked memory)");
    if (int r = set_dev(c)) return r;
    if (!c->copy_stream) {
        HIP_TRY(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&c->ev_read_ready, hipEventDisableTiming));
        for (hipEvent_t& e : c->ev_read_done) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    const int t = c->read_issued, slot = t & 7;
    if (t >= 8) HIP_TRY(hipEventSynchronize(c->ev_read_done[slot]));      // ticket t - 8 gives up its slot: its copy must have landed
    HIP_TRY(hipEventRecord(c->ev_read_ready, c->stream));
    HIP_TRY(hipStreamWaitEvent(c->copy_stream, c->ev_read_ready, 0));
    HIP_TRY(hipMemcpyAsync(dst, p, n, hipMemcpyDeviceToHost, c->copy_stream));
    HIP_TRY(hipEventRecord(c->ev_read_done[slot], c->copy_stream));
    c->read_pending[which] = t;
    c->read_issued = t + 1;
    *ticket = t;
    return RTPBR_OK;
}

extern "C" int rtpbr_read_wait(rtpbr_ctx* c, int ticket) {
    if (!c) return fail(RTPBR_EINVAL, "null ctx");
    if (ticket < 0 || ticket >= c->read_issued) return fail(RTPBR_EINVAL, "rtpbr_read_wait: no such ticket");
    if (ticket + 8 < c->read_issued) return RTPBR_OK;      // its slot was handed on, after its copy had landed
    if (int r = set_dev(c)) return r;
    HIP_TRY(hipEventSynchronize(c->ev_read_done[ticket & 7]));
    return RTPBR_OK;
}

extern "C" int rtpbr_host_alloc(rtpbr_ctx* c, size_t nbytes, void** ptr) {
    if (!c || !ptr || nbytes == 0) return fail(RTPBR_EINVAL, "rtpbr_host_alloc: context, size and result pointer are required");
    if (int r = set_dev(c)) return r;
    void* p = nullptr;
    HIP_TRY(hipHostMalloc(&p, nbytes, hipHostMallocDefault));
    c->host_blocks.push_back(p);
    c->host_sizes.push_back(nbytes);
    *ptr = p;
    return RTPBR_OK;
}

extern "C" int rtpbr_host_free(rtpbr_ctx* c, void* ptr) {
    if (!c || !ptr) return fail(RTPBR_EINVAL, "rtpbr_host_free: context and pointer are required");
    for (size_t i = 0; i < c->host_blocks.size(); i++)
        if (c->host_blocks[i] == ptr) {
            if (int r = set_dev(c)) return r;
            HIP_TRY(hipStreamSynchronize(c->stream));      // (a copy into it may be in flight)
            if (c->copy_stream) HIP_TRY(hipStreamSynchronize(c->copy_stream));
            c->host_blocks.erase(c->host_blocks.begin() + (long)i);
            c->host_sizes.erase(c->host_sizes.begin() + (long)i);
            HIP_TRY(hipHostFree(ptr));
            return RTPBR_OK;
        }
    return fail(RTPBR_EINVAL, "rtpbr_host_free: not a block of this context");
}

extern "C" int rtpbr_write_buffer(rtpbr_ctx* c, int which, const void* src, size_t nbytes) {
    void* p;
    size_t n;
    if (c && which >= 0 && which < RT_PUBLIC_BUFFERS && !((RT_WRITABLE_BUFFERS >> which) & 1u))
        return fail(RTPBR_EINVAL, "the feature, denoise, motion, moments, noise, selection, present, half, error, blend-weight, blend-depth and blend-error buffers are outputs only");
    if (int r = buf_ptr(c, which, &p, &n)) return r;
    if (!src || nbytes != n) return fail(RTPBR_EINVAL, "source size does not match the buffer");
    if (int r = set_dev(c)) return r;
    if (int r = flush_shade(c)) return r;
    if (int r = rt_order_after_reads(c, 1u << which)) return r;
    HIP_TRY(hipMemcpyAsync(p, src, n, hipMemcpyHostToDevice, c->stream));
    if (which == RTPBR_BUF_IMAGE_BUFFER && c->noise_snapshot)      // written data is no batch of the noise estimate
        HIP_TRY(hipMemcpyAsync(c->noise_snapshot, c->image_buffer, n, hipMemcpyDeviceToDevice, c->stream));
    if (which == RTPBR_BUF_IMAGE_BUFFER)                           // ... and none of the halves: it lies in B
        if (int r = half_restart(c, true)) return r;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return RTPBR_OK;
}

extern "C" int rtpbr_packed_bytes(rtpbr_ctx* c, size_t* nbytes) {
    if (!c || !nbytes || !c->have_cfg) return fail(RTPBR_ESTATE, "set_config first");
    *nbytes = (size_t)c->P.np * sizeof(float4);
    return RTPBR_OK;
}

extern "C" int rtpbr_pack_tiles(rtpbr_ctx* c, void* device_dst) {
    if (!c || !device_dst || !c->have_cfg) return fail(RTPBR_EINVAL, "bad pack_tiles arguments");
    if (int r = set_dev(c)) return r;
    c->P.cfg = c->cfg;
    c->P.image_buffer = c->image_buffer;
    launch_pack(c->P, (float4*)device_dst, c->stream);
    HIP_TRY(hipGetLastError());
    return RTPBR_OK;
}

extern "C" int rtpbr_unpack_tiles(rtpbr_ctx* c, const void* device_src, int src_rank) {
    if (!c || !device_src || !c->have_cfg) return fail(RTPBR_EINVAL, "bad unpack_tiles arguments");
    if (src_rank < 0 || src_rank >= c->world) return fail(RTPBR_EINVAL, "src_rank out of range");
    if (int r = set_dev(c)) return r;
    if (int r = rt_order_after_reads(c, W_IMAGE_BUFFER)) return r;
    Params P = c->P;
    P.cfg = c->cfg;
    P.image_buffer = c->image_buffer;
    P.rank = src_rank;
    launch_unpack(P, (const float4*)device_src, c->stream);
    HIP_TRY(hipGetLastError());
    return RTPBR_OK;
}

// the kernels add the six work counters up in 64 shards (rt_types.hpp Counters::shard): fold them into the fields
static void fold_shards(Counters& h) {
    unsigned long long* f[6] = {&h.march_steps, &h.raycasts, &h.hits, &h.sky_lookups, &h.samples, &h.deposits};
    for (int s = 0; s < 64; s++)
        for (int k = 0; k < 6; k++) *f[k] += h.shard[s][k];
}

extern "C" int rtpbr_get_counters(rtpbr_ctx* c, rtpbr_counters* out) {
    if (!c || !out) return fail(RTPBR_EINVAL, "null argument");
    if (int r = set_dev(c)) return r;
    if (int r = flush_shade(c)) return r;
    Counters h;
    HIP_TRY(hipMemcpyAsync(&h, c->counters, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    fold_shards(h);
    out->samples = h.samples;
    out->raycasts = h.raycasts;
    out->march_steps = h.march_steps;
    out->hits = h.hits;
    out->sky_lookups = h.sky_lookups;
    out->deposits = h.deposits;
    return RTPBR_OK;
}

// Named counters of the last rtpbr_sample() call: the six of rtpbr_counters plus "mlp_wave_evals" (32-ray half passes of the
// wave-cooperative neural-SDF MLP) and "mlp_lane_evals" (ray evaluations those passes were needed for).
extern "C" int rtpbr_get_counter(rtpbr_ctx* c, const char* name, unsigned long long* out) {
    if (!c || !name || !out) return fail(RTPBR_EINVAL, "null argument");
    if (int r = set_dev(c)) return r;
    if (int r = flush_shade(c)) return r;
    if (!strncmp(name, "select_tier", 11) && name[11] >= '0' && name[11] <= '7' && !name[12]) {
        // the pixels in that tier of the current selection, as its select call read them back (no copy, no synchronisation): 0 for
        // the tiers the selection does not have and before any selection; a binary selection is all tier 0
        const int t = name[11] - '0';
        *out = c->have_selection && t < c->sel_tiers ? c->sel_cum[t] - (t > 0 ? c->sel_cum[t - 1] : 0u) : 0u;
        return RTPBR_OK;
    }
    Counters h;
    HIP_TRY(hipMemcpyAsync(&h, c->counters, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    fold_shards(h);
    if (!strcmp(name, "samples")) *out = h.samples;
    else if (!strcmp(name, "raycasts")) *out = h.raycasts;
    else if (!strcmp(name, "march_steps")) *out = h.march_steps;
    else if (!strcmp(name, "hits")) *out = h.hits;
    else if (!strcmp(name, "sky_lookups")) *out = h.sky_lookups;
    else if (!strcmp(name, "deposits")) *out = h.deposits;
    else if (!strcmp(name, "mlp_wave_evals")) *out = h.mlp_wave_evals;
    else if (!strcmp(name, "mlp_lane_evals")) *out = h.mlp_lane_evals;
    else if (!strncmp(name, "dbg", 3) && name[3] >= '0' && name[3] <= '9' && !name[4]) *out = h.dbg[name[3] - '0'];
    else if (!strncmp(name, "dbg", 3) && name[3] >= 'a' && name[3] <= 'v' && !name[4]) *out = h.dbg[10 + name[3] - 'a'];
    else if (!strcmp(name, "dense_launches")) *out = c->dense_launches;      // complete-path launches of the last rtpbr_sample() that staged densely (option stage_dense)
    else if (!strncmp(name, "plan_ge:", 8)) {
        // pixels whose recorded cost was at least <n> march steps when the current plan was made (whole buckets)
        *out = 0;
        if (c->plan && c->order_valid) {
            const unsigned long long thr = strtoull(name + 8, nullptr, 10);
            PlanBuf pb;
            HIP_TRY(hipMemcpy(&pb, c->plan, sizeof pb, hipMemcpyDeviceToHost));
            for (unsigned b = 1; b < 256; b++) {
                const unsigned e = (b - 1u) >> 3, m = (b - 1u) & 7u;
                const unsigned long long fl = e >= 3u ? (unsigned long long)(8u + m) << (e - 3u) : (8u + m) >> (3u - e);
                if (fl >= thr) *out += pb.hist[b];
            }
        }
    }
    else if (!strcmp(name, "plan_heavy") || !strcmp(name, "plan_total")) {
        // the src/ pool kernel's current plan: pixels walked by heavy waves / march steps on record when it was made
        *out = 0;
        if (c->plan && c->order_valid) {
            PlanBuf pb;
            HIP_TRY(hipMemcpy(&pb, c->plan, sizeof pb, hipMemcpyDeviceToHost));
            *out = name[5] == 'h' ? pb.n_heavy : pb.total;
        }
    }
    else if (!strcmp(name, "jit_active")) *out = c->jit_mod ? 1 : 0;      // the last sample() ran a run-time compiled instance
    else if (!strcmp(name, "fill_filled") || !strcmp(name, "fill_empty") || !strcmp(name, "fill_deepest")) {
        // the last rtpbr_denoise with option denoise_fill = 1, rtpbr_denoise_coverage with option coverage_fill = 1 or level blend call
        // with option blend_fill = 1 (image_buffer's chain), iterations > 0, as its kernels counted (0 before any)
        *out = 0;
        if (c->fill_counts) {
            uint32_t sh[FILL_SHARDS * FILL_SHARD_WORDS];
            HIP_TRY(hipMemcpyAsync(sh, c->fill_counts, sizeof sh, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            const int word = name[5] == 'f' ? 0 : name[5] == 'e' ? 1 : 2;
            for (int s = 0; s < FILL_SHARDS; s++) {
                const uint32_t v = sh[s * FILL_SHARD_WORDS + word];
                *out = word == 2 ? (v > *out ? v : *out) : *out + v;
            }
        }
    }
    else if (!strcmp(name, "blend_resolved")) {
        // the pixels the resolve changed in the last rtpbr_denoise_blend_levels / rtpbr_blend_error / rtpbr_blend_error_display with
        // option blend_coverage = 1 and iterations > 0 (0 before any)
        *out = 0;
        if (c->blend_resolved) {
            uint32_t v = 0;
            HIP_TRY(hipMemcpyAsync(&v, c->blend_resolved, sizeof v, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            *out = v;
        }
    }
    else return fail(RTPBR_EINVAL, "unknown counter %s", name);
    return RTPBR_OK;
}

extern "C" int rtpbr_last_sample_ms(rtpbr_ctx* c, float* trace_ms, float* total_ms, int* launches) {
    if (!c) return fail(RTPBR_EINVAL, "null ctx");
    if (!c->timed) return fail(RTPBR_ESTATE, "no timed rtpbr_sample() call yet (option timing = 0 records no events)");
    if (int r = set_dev(c)) return r;
    HIP_TRY(hipStreamSynchronize(c->stream));
    float tr = 0.0f;
    for (int i = 0; i + 1 < c->ev_used; i += 2) {
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, c->ev[i], c->ev[i + 1]));
        tr += ms;
    }
    float tot = 0.0f;
    if (c->ev_used >= 2) {
        hipEvent_t first = c->evp_used > 0 ? c->evp[0] : c->ev[0];
        HIP_TRY(hipEventElapsedTime(&tot, first, c->total1_recorded ? c->ev_total1 : c->ev[c->ev_used - 1]));
    }
    if (trace_ms) *trace_ms = tr;
    if (total_ms) *total_ms = tot;
    if (launches) *launches = c->ev_used / 2;
    return RTPBR_OK;
}

extern "C" int rtpbr_last_primary_ms(rtpbr_ctx* c, float* primary_ms, int* launches) {
    if (!c) return fail(RTPBR_EINVAL, "null ctx");
    if (!c->timed) return fail(RTPBR_ESTATE, "no timed rtpbr_sample() call yet (option timing = 0 records no events)");
    if (int r = set_dev(c)) return r;
    HIP_TRY(hipStreamSynchronize(c->stream));
    float pr = 0.0f;
    for (int i = 0; i + 1 < c->evp_used; i += 2) {
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, c->evp[i], c->evp[i + 1]));
        pr += ms;
    }
    if (primary_ms) *primary_ms = pr;
    if (launches) *launches = c->evp_used / 2;
    return RTPBR_OK;
}

extern "C" int rtpbr_get_stream(rtpbr_ctx* c, void** stream) {
    if (!c || !stream) return fail(RTPBR_EINVAL, "null argument");
    *stream = (void*)c->stream;
    return RTPBR_OK;
}

// The plain integer options: the key is the member's name, a value outside lo..hi is refused in the row's words.  replan: the
// plan of the src/ pool kernel was made for the old value (order_valid, cost_steps).
struct OptionRow {
    const char* key;
    int rtpbr_ctx::*member;
    long long lo, hi;
    bool replan;
    const char* refusal;
};
#define OPTION(member, lo, hi, replan, refusal) {#member, &rtpbr_ctx::member, lo, hi, replan, refusal}
static const OptionRow OPTION_ROWS[] = {
    OPTION(wait_lanes, 1, 64, false, "wait_lanes must be 1..64"),
    OPTION(shade_lanes, 1, 64, false, "shade_lanes must be 1..64"),
    OPTION(jit_waves, 0, 8, false, "jit_waves must be 0 (default) .. 8"),
    // every wave makes one claim past the end, so the 32-bit work counter overshoots by waves x chunk: the margin kept
    // free below 2^32 (work_margin) covers 32 waves per CU x 8192
    OPTION(chunk, 0, 8192, false, "chunk must be 0 (automatic) .. 8192"),
    OPTION(sparse_lanes, 0, 64, false, "sparse_lanes must be 0 (never) .. 64"),
    OPTION(src_plan, 0, 1, true, "src_plan must be 0 or 1"),
    OPTION(plan_interval, 1, 1 << 20, false, "plan_interval must be 1 .. 2^20 bounce-steps"),
    OPTION(heavy_own, 0, 128, true, "heavy_own must be 0 (no heavy waves) .. 128"),      // the plan's share of heavy pixels was sized for the old value
    OPTION(chain_waves, 1, 2048, true, "chain_waves must be 1 .. 2048"),
    OPTION(src_split, 0, 256, false, "src_split must be 0 (never) .. 256 (bounce-steps per launch up to which the wavefront split runs)"),
    OPTION(env_packed, 0, 1, false, "env_packed must be 0 (float4 texels) or 1 (RGBA8 texels + 256-entry table: 8-bit sources, same values)"),
    OPTION(src_lazy, 0, 1, false, "src_lazy must be 0 (every one-step launch shades) or 1 (the shading rides with the next launch's gen pass)"),
    OPTION(split_head, -1, 1, false, "split_head must be -1 (automatic: small frames), 0 (the heavy head fills the first groups) or 1 (interleaved: one head entry per group)"),
    OPTION(split_wait, 1, 64, false, "split_wait must be 1..64"),
    OPTION(src_track, 0, 2, false, "src_track must be 0 (never), 1 (one-object bounds only) or 2 (one- and two-object bounds)"),
    OPTION(src_op, 0, 7, false, "src_op must be 0 .. 7 (bit 0: object-parallel evaluation for sparse waves in the split march and chain kernels, bit 1: in the fused pool kernel, bit 2: the per-lane lean loop for lanes that track different objects)"),
    OPTION(tiny_waves, 0, 65535, false, "tiny_waves must be 0 .. 65535"),
    OPTION(tiny_own, 0, 128, false, "tiny_own must be 0 (no small heavy waves) .. 128"),
    OPTION(leave_x8, 1, 4096, false, "leave_x8 must be 1 .. 4096 (eighths of a march iteration)"),
    OPTION(heavy_prio, 0, 1, false, "heavy_prio must be 0 or 1"),
    OPTION(heavy_mean_x16, 0, 1 << 20, false, "heavy_mean_x16 must be 0 .. 2^20"),
    OPTION(heavy_bulk_x16, 0, 1 << 20, false, "heavy_bulk_x16 must be 0 .. 2^20"),
    OPTION(grid_blocks, 0, 65535, false, "grid_blocks must be 0 (automatic) .. 65535"),
    OPTION(cover_blocks, 0, 65535, false, "cover_blocks must be 0 (automatic) .. 65535"),
    OPTION(denoise_fill, 0, 1, false, "denoise_fill must be 0 (pixels without samples stay as rtpbr_post_process shows them) or 1 (rtpbr_denoise reconstructs them from their neighbours)"),
    OPTION(coverage_fill, 0, 1, false, "coverage_fill must be 0 (pixels without samples stay as rtpbr_post_process shows them) or 1 (rtpbr_denoise_coverage reconstructs them from their neighbours)"),
    OPTION(blend_coverage, 0, 1, false, "blend_coverage must be 0 (the plain filter's ladders) or 1 (rtpbr_denoise_blend_levels, rtpbr_blend_error and rtpbr_blend_error_display run the coverage-weighted ladders and the edge resolve)"),
    OPTION(blend_fill, 0, 1, false, "blend_fill must be 0 (pixels without samples stay as rtpbr_post_process shows them) or 1 (rtpbr_denoise_blend_levels, rtpbr_blend_error and rtpbr_blend_error_display reconstruct them from their neighbours)"),
    // read by the select calls only: a selection keeps the tiers it was built with (rt_select.hpp, include/rtpbr.h)
    OPTION(select_tiers, 1, 8, false, "select_tiers must be 1 (every selected pixel takes the whole batch of rtpbr_sample_selected) .. 8 (the select calls give every selected pixel one of that many shares of it)"),
    OPTION(select_batch, 1, 65536, false, "select_batch must be 1 .. 65536 (the n the host will pass to rtpbr_sample_selected: with select_tiers > 1 the noise-driven select calls size the shares by it)"),
    OPTION(blend_coverage_grid, 2, 4, false, "blend_coverage_grid must be 2 or 4"),      // (3: refused in rtpbr_set_option)
    OPTION(blend_coverage_power, 0, 8, false, "blend_coverage_power must be 0..8"),
    OPTION(blend_coverage_resolve, 0, 1, false, "blend_coverage_resolve must be 0 or 1"),
    OPTION(ready_low, 0, 63, false, "ready_low must be 0..63"),
    OPTION(refill_lanes, 1, 64, false, "refill_lanes must be 1..64"),
    // 1 (default): rtpbr_sample() brackets its kernels with events (rtpbr_last_sample_ms / rtpbr_last_primary_ms); 0: none — an event
    // is a barrier packet with a completion signal, and four of them cost a launch of a few hundred microseconds a fifth of its time
    OPTION(timing, 0, 1, false, "timing must be 0 or 1"),
    OPTION(stage_dense, 0, 1, false, "stage_dense must be 0 (item-linear staging) or 1 (records appended per claim in completion order)"),
    OPTION(primary_split, 0, 2, false, "primary_split must be 0 (never), 1 (large launches) or 2 (always)"),
    OPTION(drain_lanes, 0, 64, false, "drain_lanes must be 0..64"),
    OPTION(primary_lean, 0, 1, false, "primary_lean must be 0 or 1"),
    OPTION(lazy_sqrt, 0, 1, false, "lazy_sqrt must be 0 or 1"),
    OPTION(jit, -1, 2, false, "jit must be -1 (when no ahead-of-time specialisation fits), 0 (never), 1 (always, falling back to the "
                              "ahead-of-time instance if compilation is impossible) or 2 (always, an error otherwise)"),
    OPTION(precision, 0, 1, false, "precision must be 0 (exactly rounded, the default) or 1 (tolerance flavour: hardware sqrt / rcp / sin / exp, contraction)"),
    OPTION(jit_bake, 0, 2, false, "jit_bake must be 0, 1 (scene + configuration) or 2 (+ the camera frame: fixed-camera offline renders)"),
    OPTION(specialize, 0, 1, false, "specialize must be 0 or 1"),
    OPTION(mlp_mfma, 0, 1, false, "mlp_mfma must be 0 or 1"),
    OPTION(mlp_lanes, 1, 64, false, "mlp_lanes must be 1..64"),
    OPTION(mlp_full, 1, 65, false, "mlp_full must be 1..65 (65 = never compute both halves at once)"),
    OPTION(swap_lanes, 0, 64, false, "swap_lanes must be 0 (automatic: 8 in the complete-path pool kernel, 12 in the src/ one) .. 64"),
    OPTION(scheduler, -1, 1, false, "scheduler must be -1 (auto), 0 or 1"),
    OPTION(waves_per_cu, 0, 32, false, "waves_per_cu must be 0..32"),
};
#undef OPTION

extern "C" int rtpbr_set_option(rtpbr_ctx* c, const char* key, long long value) {
    if (!c || !key) return fail(RTPBR_EINVAL, "null argument");
    if (int r = flush_shade(c)) return r;
    for (const OptionRow& o : OPTION_ROWS)
        if (!strcmp(key, o.key)) {
            if (value < o.lo || value > o.hi) return fail(RTPBR_EINVAL, o.refusal);
            if (o.member == &rtpbr_ctx::blend_coverage_grid && value == 3) return fail(RTPBR_EINVAL, o.refusal);      // (the one row with a gap)
            c->*o.member = (int)value;
            if (o.replan) {
                c->order_valid = false;
                c->cost_steps = 0;
            }
            return RTPBR_OK;
        }
    // the options that are more than a number within bounds
    if (!strcmp(key, "staging_bytes")) {
        if (value < (1 << 20)) return fail(RTPBR_EINVAL, "staging_bytes must be >= 1 MiB");
        c->staging_bytes = value;
    } else if (!strcmp(key, "src_chain")) {
        if (value < 0 || value > 2) return fail(RTPBR_EINVAL, "src_chain must be 0 (never), 1 (when the device has room beside the pool kernel) or 2 (always: tests)");
        c->src_chain = (int)value;
        c->order_valid = false;       // the plan carries the chain set
        c->cost_steps = 0;
        c->plan_chain_waves = 0;
        c->plan_rb_pending = false;
    } else if (!strcmp(key, "chain_np_max")) {
        if (value < 0) return fail(RTPBR_EINVAL, "chain_np_max must be >= 0");
        c->chain_np_max = value;
    } else if (!strcmp(key, "age_weights")) {
        // one hex digit per residency slot, oldest first (0x88888 = equal shares); 0 switches the weighting off
        if (value < 0 || value > 0xffffffffLL) return fail(RTPBR_EINVAL, "age_weights must be 0 (off) or up to 8 hex digits, one per residency slot");
        c->age_on = value != 0 ? 2 : 0;
        int nd = 0;
        for (long long v = value; v; v >>= 4) nd++;
        for (int k = 0; k < 8; k++) c->age_w[k] = k < nd ? (int)((value >> (4 * (nd - 1 - k))) & 15) : 8;
        for (int k = 0; k < 8; k++)
            if (c->age_w[k] == 0) c->age_w[k] = 1;
    } else if (!strcmp(key, "age_tune")) {
        if (value < 0 || value > 1) return fail(RTPBR_EINVAL, "age_tune must be 0 (equal shares) or 1 (self-tuned age-weighted shares)");
        c->age_on = (int)value;
    } else if (!strcmp(key, "residency")) {
        if (value < 1 || value > 256 || (value & (value - 1))) return fail(RTPBR_EINVAL, "residency must be a power of two, 1..256");
        c->residency = (int)value;
    } else if (!strcmp(key, "reserve_spp")) {
        // allocate the staging of a `value`-spp rtpbr_sample() call now (complete-path form)
        if (!c->have_cfg || c->P.np <= 0) return fail(RTPBR_ESTATE, "set_config (and set_tiles) first");
        if (value < 1) return fail(RTPBR_EINVAL, "reserve_spp must be >= 1");
        if (int r = set_dev(c)) return r;
        const bool split_ok = c->primary_split && c->scheduler != 0 && !(c->have_scene && (c->kind == KIND_BUNNY || c->kind == KIND_MIXED));
        const bool unstaged = c->precision != 0 && c->scheduler != 0;      // the tolerance flavour has no staging (rtpbr_sample)
        const long long K = staging_plan(c->P.np, value, c->staging_bytes, c->n_cu, split_ok, unstaged, c->primary_split).K;
        if (int r = ensure_staging(c, (size_t)c->P.np * (size_t)K, split_ok, !unstaged))
            return r == RTPBR_ENOMEM ? fail(RTPBR_ENOMEM, "reserve_spp: no device memory for the staging of that many samples per pixel") : r;
    } else if (!strcmp(key, "select_lattice")) {
        // build the selection of a lattice now, on the device (a command, as reserve_spp is)
        return select_lattice_option(c, value);
    } else if (!strcmp(key, "sample_base")) {
        c->sample_base = (uint32_t)value;
    } else {
        return fail(RTPBR_EINVAL, "unknown option %s", key);
    }
    return RTPBR_OK;
}

// test hook: exact math functions evaluated on the device (not part of the drop-in surface)
extern "C" int rtpbr_test_math(rtpbr_ctx* c, int op, const float* a, const float* b, float* out, float* out2, int n) {
    if (!c || !a || !out || n <= 0) return fail(RTPBR_EINVAL, "bad test_math arguments");
    if (int r = set_dev(c)) return r;
    float *da = nullptr, *db = nullptr, *dout = nullptr, *dout2 = nullptr;
    size_t nb = (size_t)n * sizeof(float);
    const int rc = [&]() -> int {      // (every return leaves through the frees below)
        HIP_TRY(hipMalloc(&da, nb));
        HIP_TRY(hipMalloc(&dout, nb));
        HIP_TRY(hipMalloc(&dout2, nb));
        HIP_TRY(hipMemcpy(da, a, nb, hipMemcpyHostToDevice));
        if (b) {
            HIP_TRY(hipMalloc(&db, nb));
            HIP_TRY(hipMemcpy(db, b, nb, hipMemcpyHostToDevice));
        }
        launch_math_probe(op, da, db, dout, dout2, n, c->stream);
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipMemcpy(out, dout, nb, hipMemcpyDeviceToHost));
        if (out2) HIP_TRY(hipMemcpy(out2, dout2, nb, hipMemcpyDeviceToHost));
        return RTPBR_OK;
    }();
    (void)hipFree(da);
    (void)hipFree(db);
    (void)hipFree(dout);
    (void)hipFree(dout2);
    return rc;
}

// test hook: exhaustive check of the device sqrt_ against IEEE sqrt; *mismatches must come back 0
extern "C" int rtpbr_test_sqrt_exhaustive(rtpbr_ctx* c, unsigned long long* mismatches) {
    if (!c || !mismatches) return fail(RTPBR_EINVAL, "null argument");
    if (int r = set_dev(c)) return r;
    unsigned long long* d = nullptr;
    HIP_TRY(hipMalloc(&d, sizeof *d));
    const int rc = [&]() -> int {      // (every return leaves through the free below)
        HIP_TRY(hipMemset(d, 0, sizeof *d));
        launch_sqrt_exhaustive(d, c->stream);
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipMemcpy(mismatches, d, sizeof *d, hipMemcpyDeviceToHost));
        return RTPBR_OK;
    }();
    (void)hipFree(d);
    return rc;
}
