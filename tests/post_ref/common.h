/* post_ref section: what every post stage's restatement is made of.  f32, nothing fused; sums run dy outer, dx inner. */
#define POST_API __attribute__((visibility("default")))

static inline float lum(const float* c) { return (0.299f * c[0] + 0.587f * c[1]) + 0.114f * c[2]; }
static inline float lum3(v3 c) { return (0.299f * c.x + 0.587f * c.y) + 0.114f * c.z; }
static inline float sq3(v3 v) { return (v.x * v.x + v.y * v.y) + v.z * v.z; }
static inline v3 load3(const float* c) { return v3_make(c[0], c[1], c[2]); }
static inline void store3(float* o, v3 c) { o[0] = c.x; o[1] = c.y; o[2] = c.z; }
/* c / (1 + c): the range map of the filter's colour distance and of the noise estimate */
static inline v3 range_map(v3 c) { return v3_make(c.x / (1.0f + c.x), c.y / (1.0f + c.y), c.z / (1.0f + c.z)); }
static inline v3 demodulated(v3 c, const float* a) {
    return v3_make(c.x / fmaxf(a[0], 1e-3f), c.y / fmaxf(a[1], 1e-3f), c.z / fmaxf(a[2], 1e-3f));
}
static inline v3 remodulated(v3 c, const float* a) {
    return v3_make(c.x * fmaxf(a[0], 1e-3f), c.y * fmaxf(a[1], 1e-3f), c.z * fmaxf(a[2], 1e-3f));
}
static inline v3 tone_map3(const rtpbr_config* cfg, const float* c3) {
    const float c[4] = {c3[0], c3[1], c3[2], 1.0f};
    return tone_map(cfg, c);
}

/* one more pixel in stats = {pixels_estimated, pixels_above, bits of the largest value} (zeroed by the caller) */
static inline void stats_fold(uint32_t* stats, float value, float threshold) {
    uint32_t bits;
    memcpy(&bits, &value, 4);
    stats[0]++;
    if (value > threshold) stats[1]++;
    if (bits > stats[2]) stats[2] = bits;
}

/* (u, v) of the centre of pixel (x, y) as the camera kinds compute it */
static inline void pixel_uv(const rtpbr_config* cfg, int x, int y, float* u, float* v) {
    const int W = cfg->width, H = cfg->height;
    if (cfg->camera_kind == RTPBR_CAMERA_PINHOLE) {
        *u = ((float)x + 0.5f) / (float)W;
        *v = ((float)y + 0.5f) / (float)H;
    } else {
        *u = ((float)x + 0.5f) * (1.0f / (float)W);
        *v = ((float)y + 0.5f) * (1.0f / (float)H);
    }
}

/* The window walk: the statement after it runs for every tap (dx, dy) of the (2r + 1)^2 window around (x, y), taps `step` pixels
 * apart, that lies in the W x H frame, with q its index; dy outer, dx inner.  `continue` in the statement goes on to the next tap. */
#define FOR_WINDOW(q, r, step, x, y, W, H)                                                      \
    for (int dy = -(r); dy <= (r); dy++)                                                        \
        for (int dx = -(r), yq_ = (y) + (step) * dy; dx <= (r) && yq_ >= 0 && yq_ < (H); dx++)  \
            for (int xq_ = (x) + (step) * dx, in_ = xq_ >= 0 && xq_ < (W); in_; in_ = 0)        \
                for (const size_t q = (size_t)xq_ * (H) + yq_; in_; in_ = 0)
