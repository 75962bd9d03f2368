/*
 * post_ref.c — the CPU restatements of the post stages that need the oracle (TEST INFRASTRUCTURE ONLY): features and denoise,
 * reprojection, noise, the half mode, and the blends with their error estimates.
 *
 * One translation unit: the oracle's source is included once for its camera frame, raycasts, tone map and math (the oracle itself
 * is not changed), then the sections.  tests/ref_build.py builds it on demand with the oracle's flags (-ffp-contract=off) plus
 * -fvisibility=hidden -Wl,-Bsymbolic: the library carries its own copy of every rto_* symbol and of the bunny weights, which must
 * not interpose with librt_oracle.so, loaded RTLD_GLOBAL in the same process.  Only the POST_API functions are exported; the
 * wrapper modules of tests/ (feature_ref_lib.py and its kin) bind to them.  The arithmetic follows include/rtpbr.h operation by operation.
 */
#include "../../oracle/rt_oracle.c"

#include "common.h"      /* luminance, range map, modulation, the statistics fold, the window walk */
#include "features.h"    /* fr_features */
#include "filter.h"      /* the a-trous filter: fr_denoise, br_filter, lr_filter_levels, nr_guided */
#include "noise.h"       /* nr_update, nr_estimate */
#include "gather.h"      /* the bilinear gather: rr_reproject, nr_reproject, rs_moved, rs_reproject_scene, hm_gather */
#include "half_mode.h"   /* hm_fold */
#include "blend.h"       /* the blend rule: br_blend, lr_blend_levels, ber_blend_error */
