/*
 * mvs_scene_prep.h — the scene-preparation entries of libmvs_hip.so (csrc/scene_prep.hip), a companion of mvs_hip.h: same library, same
 * conventions (return 0 / MVS_EINVAL / -(1000 + hipError_t), mvs_last_error(), device pointers owned by the caller, asynchronous on
 * `stream`, nothing allocated).  A header of its own because the entries are additions that leave mvs_hip.h, its ABI number (51) and the
 * table bound from it exactly as they were; mvsformer_amd/_lib.py binds this header's prototypes the same way, from this text.
 *
 * From a sparse reconstruction to what `pair.txt` and the depth-range row of a `*_cam.txt` hold - the step BEFORE the pipeline, which the
 * reference leaves to MVSNet's `colmap2mvsnet.py` ("you should build a new pair.txt with 20 views as MVSNet").  That script is not part
 * of the reference: the rule below is RESTATED from memory of the published script, every constant is an argument, and
 * parity with the original script is UNVERIFIED.
 *
 * Inputs: xyz [N][3] fp32 points; one observation per track element, (obs_point [M] int64, obs_view [M] int32); R [V][3][3], t [V][3] fp32,
 * world to camera.  1 <= V <= MVS_SCENE_MAX_VIEWS, 1 <= N < 2^31, 0 <= M < 2^32 (the per-view counts and their sum are uint32).  A bitset
 * row holds Wd = ceil(N / 64) 64-bit words; bit p % 64 of word p / 64 of row v belongs to point p.  The entries that READ a bitset ignore
 * bits at or above N.
 *
 * mvs_scene_visibility    bits [V][Wd] uint64 (zeroed here first): bit p of row v is set iff some observation names (p, v) and the three
 *                         coordinates of p are finite.  64-bit atomic OR: the result does not depend on the order, duplicates collapse.
 *                         count [V] uint32 = the set bits per row.  info [2] int64 (device): [0] observations with obs_point outside [0, N) or
 *                         obs_view outside [0, V) - counted, never written through; [1] points with a non-finite coordinate.  info_host NULL:
 *                         nothing waits, the caller reads info.  info_host [2] (host): the entry waits for the stream, copies info there and
 *                         returns MVS_EINVAL when info[0] != 0.
 * mvs_scene_pair_scores   S [V][V] fp64, symmetric, zero diagonal (zeroed here first).  centers [V][3] fp64 (scratch, written here):
 *                         C_k = -((R[0][k] t0 + R[1][k] t1) + R[2][k] t2).  For i < j,
 *                           S[i][j] = S[j][i] = sum over the points p set in row i AND row j of g(theta_ij(p)),
 *                           a = C_i - p, b = C_j - p, c = a x b,
 *                           theta = atan2(sqrt((c0 c0 + c1 c1) + c2 c2), (a0 b0 + a1 b1) + a2 b2) * (180 / pi)      [degrees, in [0, 180]]
 *                           g = exp(-((theta - theta0) (theta - theta0)) / (2 sigma sigma)),  sigma = sigma1 if theta <= theta0 else sigma2,
 *                         all in fp64, uncontracted (the script takes acos of the normalised dot product; atan2 is the same angle, well
 *                         conditioned near 0, and atan2(0, 0) = 0 makes a point on a camera centre a term, not a NaN).  The script's
 *                         constants: theta0 = 5, sigma1 = 1, sigma2 = 10.  Order of the additions: one wavefront per pair; lane l walks the
 *                         words l, l + 64, ... of (row i & row j) and the set bits of a word in ascending order, adding into its own sum;
 *                         then the wavefront's shuffle tree (32, 16, ... 1).  No atomics: S depends on the input alone.
 * mvs_scene_rank_sources  src [V][k] int32, score [V][k] fp64: for view i the views j != i in descending S[i][j], equal scores in ascending
 *                         j (what a stable descending sort leaves): slot rank(j) = #{m != i : S[i][m] > S[i][j] or (S[i][m] == S[i][j] and
 *                         m < j)} takes (j, S[i][j]) when rank(j) < k.  Slots past V - 2: (-1, 0).  S must hold no NaN.  k >= 1.
 * mvs_scene_depth_ranges  per view v the depths z = ((R[v][2][0] x + R[v][2][1] y) + R[v][2][2] z) + t[v][2] of the points set in row v, in
 *                         fp32, each operation rounded on its own in this order (numpy float32 reproduces it bit for bit), compacted in
 *                         ascending point order into depths [offsets[v], offsets[v + 1]); offsets [V + 1] int64 = the exclusive scan of
 *                         count (both scratch, written here; depths holds `capacity` floats, the sum of count fits when capacity >= the
 *                         number of observations).  n [V] int32 = count[v];  range [V][2] fp32 = (sorted[min(int(n lo), n - 1)],
 *                         sorted[min(int(n hi), n - 1)]) with n lo formed in fp64 - an exact selection (four 8-bit histogram passes over the
 *                         order-preserving uint32 key of the float: negative depths order below positive ones, -0 below +0, NaN above
 *                         +inf), no sort.  The script's constants: lo = 0.01, hi = 0.99 (0 <= lo <= hi <= 1).  A view with no point:
 *                         range (0, 0), n = 0, no error.  A view whose segment would end past `capacity`, or whose row does not hold
 *                         count[v] bits: range (0, 0), n = -1, nothing of it is written.
 */
#ifndef MVS_SCENE_PREP_H
#define MVS_SCENE_PREP_H

#include "mvs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MVS_SCENE_MAX_VIEWS 8192
int mvs_scene_visibility(const int64_t* obs_point, const int32_t* obs_view, int64_t M, const float* xyz, int64_t N, int V, uint64_t* bits,
                         uint32_t* count, int64_t* info, int64_t* info_host, mvs_stream_t stream);
int mvs_scene_pair_scores(const uint64_t* bits, const float* xyz, int64_t N, const float* R, const float* t, int V, double theta0,
                          double sigma1, double sigma2, double* centers, double* S, mvs_stream_t stream);
int mvs_scene_rank_sources(const double* S, int V, int k, int32_t* src, double* score, mvs_stream_t stream);
int mvs_scene_depth_ranges(const uint64_t* bits, const uint32_t* count, const float* xyz, int64_t N, const float* R, const float* t, int V,
                           double lo, double hi, int64_t* offsets, float* depths, int64_t capacity, float* range, int32_t* n,
                           mvs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MVS_SCENE_PREP_H */
