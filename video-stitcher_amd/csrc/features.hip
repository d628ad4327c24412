// features.hip -- the feature front-end of the recalibration path on the device (gfx950):
//   featurefinder::findFeatures   (360_stitcher/featurefinder.cpp:13-46)  cuda::ORB::create(2500, 1.2f, 8)->detectAndCompute
//       host logic   sources/modules/cudafeatures2d/src/orb.cpp:430-865 (pyramid, per-level budgets, culls, merge)
//       kernels      cudafeatures2d/src/cuda/fast.cu:224-344 (FAST 9-16 + score + non-max suppression),
//                    cuda/orb.cu:93-138 (Harris response), :160-211 (intensity-centroid angle), :222-367 (rBRIEF, WTA_K = 2)
//   featurefinder::matchFeatures' findHomography(src, dst, mask, RANSAC)  (featurefinder.cpp:68-90)
//       calib3d/src/fundam.cpp:46-260, 319-402; ptsetreg.cpp:53-290; levmarq.cpp:76-214
//
// ORB is one device pass for every view of a rig (orb_batch and the k_ob_* kernels; ms_orb_detect_and_compute is the batch of one): image / mask pyramids,
// FAST scores, non-max suppression and ordered compaction, both culls, Harris responses, angles, descriptors.  The host builds a table from the shapes and the
// parameters (level sizes, per-level budgets, the detector's buffer, every buffer offset), uploads it, and reads the counts and keypoint rows back after ONE
// synchronisation; no count comes back between the stages (the reference reads them back per level: fast.cu:338-341, :379-382) and no cull runs on the host.
// The reference sorts with an unstable thrust sort and compacts through atomics, so its keypoint order is not defined.  Ours is: raster order after FAST, a
// stable descending sort in both culls, levels concatenated -- the order of oracle/orb_oracle.py, which the tests hold every result to byte for byte.
// RANSAC's hypothesis fitting and scoring are on the device too (all `maxIters` 4-point models of every problem of a batch at once: one lane per model fits it,
// one workgroup per 64 models counts their inliers; ms_find_homography_ransac is the batch of one).  What stays on the host there, as in the reference: the
// sequential subset draw and best-model scan, and the final N-point fit + Levenberg-Marquardt polish of ONE model.
// Conventions where CUDA leaves freedom (same as oracle/orb_oracle.py): float expressions without fma contraction; atan2f / sincosf as the
// correctly rounded float of the double function.
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>
#include "common.hpp"

namespace ms {
namespace {

struct P2 { signed char x, y; };
__constant__ P2 c_pattern[512] = {
#include "orb_pattern.inc"
};

// FAST circle in the bit order of fast.cu's masks (bit k = C[k / 4] byte k % 4): (dy, dx)
__constant__ signed char c_circ[16][2] = {{3, 0}, {3, 1}, {2, 2}, {1, 3}, {0, 3}, {-1, 3}, {-2, 2}, {-3, 1}, {-3, 0}, {-3, -1}, {-2, -2}, {-1, -3}, {0, -3}, {1, -3}, {2, -2}, {3, -1}};

// calcKeypoints<true> (fast.cu:264-307): score map, 0 = no corner.  The mask of the level = user mask AND the inner rectangle left by edgeThreshold
// (orb.cpp:707-712), applied analytically.  A pixel is a corner when 9 contiguous circle pixels are all darker than v - th or all brighter than v + th
// (the c_table lookup of fast.cu:201-206 encodes exactly "the 16-bit mask holds 9 contiguous ones": tests/test_orb_oracle.py::test_arc9_equals_the_references_table
// holds the rule to that table, tests/test_features_edges_gpu.py::test_every_16_bit_arc_mask holds this function to the rule over all 65 536 masks);
// cornerScore's binary search (fast.cu:208-222) finds the largest threshold that still passes = (best arc's smallest difference) - 1.
__device__ __forceinline__ int fast_score_at(const uint8_t *__restrict__ img, size_t step, int rows, int cols, const uint8_t *__restrict__ mask, size_t mstep, int edge, int th,
                                             int i, int j)
{
    int s = 0;
    const bool inner = i >= edge && j >= edge && i < rows - edge && j < cols - edge && cols > 2 * edge && rows > 2 * edge;
    if (i >= 3 && j >= 3 && i < rows - 3 && j < cols - 3 && inner && (!mask || mask[(size_t)i * mstep + j])) {
        const int v = img[(size_t)i * step + j];
        int d[16];
        unsigned dark = 0, bright = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            d[k] = (int)img[(size_t)(i + c_circ[k][0]) * step + (j + c_circ[k][1])] - v;
            dark |= (unsigned)(d[k] < -th) << k;
            bright |= (unsigned)(d[k] > th) << k;
        }
        auto arc9 = [](unsigned m) { unsigned a = m; for (int q = 1; q < 9; ++q) a &= ((m >> q) | (m << (16 - q))) & 0xffffu; return a != 0; };
        if (arc9(dark) || arc9(bright)) {
            int a = -32768, b = -32768;
#pragma unroll
            for (int st = 0; st < 16; ++st) {
                int mn = 32767, mx = 32767;
#pragma unroll
                for (int q = 0; q < 9; ++q) { const int dv = d[(st + q) & 15]; mn = min(mn, dv); mx = min(mx, -dv); }
                a = max(a, mn); b = max(b, mx);
            }
            s = min(max(a, b), 256) - 1;
        }
    }
    return s;
}

// nonmaxSuppression's test (fast.cu:346-371): a corner survives when its score is strictly above its 8 neighbours'
__device__ __forceinline__ bool is_local_max(const uint8_t *__restrict__ score, size_t sstep, int i, int j)
{
    const int s = score[(size_t)i * sstep + j];
    if (s == 0) return false;
    const uint8_t *r0 = score + (size_t)(i - 1) * sstep + j, *r1 = r0 + sstep, *r2 = r1 + sstep;
    return s > r0[-1] && s > r0[0] && s > r0[1] && s > r1[-1] && s > r1[1] && s > r2[-1] && s > r2[0] && s > r2[1];
}

// createMesh's feature mask (meshwarper.cpp:82-115): overlap bands AND not-black
__global__ void __launch_bounds__(256) k_feature_mask(const uint8_t *__restrict__ img, size_t step, int rows, int cols, int ax0, int ax1, int bx0, int bx1,
                                                      uint8_t *__restrict__ mask, size_t mstep)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= cols || y >= rows) return;
    const uint8_t *p = img + (size_t)y * step + 3 * (size_t)x;
    const bool band = (x >= ax0 && x < ax1) || (x >= bx0 && x < bx1);
    mask[(size_t)y * mstep + x] = (band && (p[0] | p[1] | p[2])) ? 255 : 0;
}

// ms_feature_inputs_batch: view v's images and bands (ax0 <= x < ax1 or bx0 <= x < bx1), its first workgroup and the number of 256-pixel tiles across a row.  The table
// travels as the kernel's argument: no upload, no scratch.
struct FiView { const uint8_t *src; uint8_t *gray, *mask; size_t sstep, gstep, mstep; int w, h, ax0, ax1, bx0, bx1, block0, tiles_x; };
struct FiTable { FiView v[MS_MAX_VIEWS]; int n; };

__device__ __forceinline__ void fi_store4(uint8_t *base, size_t step, int x, int y, unsigned q, int n)
{
    uint8_t *d = base + (size_t)y * step + x;
    if (n == 4 && ((step | (size_t)base) & 3) == 0) *reinterpret_cast<unsigned *>(d) = q;
    else for (int k = 0; k < n; ++k) d[k] = (uint8_t)(q >> (8 * k));
}

// cvtColor(BGR2GRAY) (featurefinder.cpp:34: CV_DESCALE(b * 1868 + g * 9617 + r * 4899, 14)) and createMesh's feature mask (meshwarper.cpp:82-115) of every view in one
// launch: a workgroup = one 256 x 4 pixel tile of one view, a lane = 4 pixels of a row, each BGR pixel read once for both outputs
__global__ void __launch_bounds__(256) k_feature_inputs(const FiTable T)
{
    int vi = 0;
    while (vi + 1 < T.n && (int)blockIdx.x >= T.v[vi + 1].block0) ++vi;
    const FiView &V = T.v[vi];
    const int local = (int)blockIdx.x - V.block0, ty = local / V.tiles_x, tx = local - ty * V.tiles_x;
    const int x = 4 * (tx * 64 + (int)threadIdx.x), y = ty * 4 + (int)threadIdx.y;
    if (x >= V.w || y >= V.h) return;
    const uint8_t *p = V.src + (size_t)y * V.sstep + (size_t)x * 3;
    const int n = min(4, V.w - x);
    uint8_t px[12];
    if (n == 4 && ((V.sstep | (size_t)V.src) & 3) == 0) __builtin_memcpy(px, __builtin_assume_aligned(p, 4), 12);
    else for (int i = 0; i < 3 * n; ++i) px[i] = p[i];
    unsigned g = 0, m = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < n) {
            const unsigned b = px[3 * k], gr = px[3 * k + 1], r = px[3 * k + 2];
            g |= ((b * 1868u + gr * 9617u + r * 4899u + (1u << 13)) >> 14) << (8 * k);
            const int xk = x + k;
            const bool band = (xk >= V.ax0 && xk < V.ax1) || (xk >= V.bx0 && xk < V.bx1);
            if (band && (b | gr | r)) m |= 255u << (8 * k);
        }
    if (V.gray) fi_store4(V.gray, V.gstep, x, y, g, n);
    if (V.mask) fi_store4(V.mask, V.mstep, x, y, m, n);
}

// HarrisResponses (orb.cu:93-138): 7 x 7 block, integer gradient sums, float formula evaluated operation by operation
__device__ __forceinline__ float harris_at(const uint8_t *__restrict__ img, size_t step, int x, int y, int block, float k)
{
    const int r = block / 2, x0 = x - r, y0 = y - r;
    int a = 0, b = 0, c = 0;
    for (int i = 0; i < block; ++i)
        for (int j = 0; j < block; ++j) {
            const uint8_t *q = img + (size_t)(y0 + i) * step + (x0 + j);
            const int ix = ((int)q[1] - (int)q[-1]) * 2 + ((int)q[1 - (ptrdiff_t)step] - (int)q[-1 - (ptrdiff_t)step]) + ((int)q[1 + step] - (int)q[step - 1]);
            const int iy = ((int)q[step] - (int)q[-(ptrdiff_t)step]) * 2 + ((int)q[step - 1] - (int)q[-(ptrdiff_t)step - 1]) + ((int)q[step + 1] - (int)q[1 - (ptrdiff_t)step]);
            a += ix * ix; b += iy * iy; c += ix * iy;
        }
    float scale = (float)(1 << 2) * (float)block * 255.0f;
    scale = 1.0f / scale;
    const float s4 = ((scale * scale) * scale) * scale;
    const float fa = (float)a, fb = (float)b, fc = (float)c, s = fa + fb;
    return ((fa * fb - fc * fc) - (k * s) * s) * s4;
}

// IC_Angle (orb.cu:160-211)
__device__ __forceinline__ float ic_angle_at(const uint8_t *__restrict__ img, size_t step, int x, int y, int half, const int *__restrict__ umax)
{
    const uint8_t *c = img + (size_t)y * step + x;
    int m01 = 0, m10 = 0;
    for (int u = -half; u <= half; ++u) m10 += u * (int)c[u];
    for (int v = 1; v <= half; ++v) {
        const int d = umax[v];
        int vs = 0, msum = 0;
        for (int u = -d; u <= d; ++u) {
            const int pl = c[(ptrdiff_t)v * (ptrdiff_t)step + u], mi = c[-(ptrdiff_t)v * (ptrdiff_t)step + u];
            vs += pl - mi; msum += u * (pl + mi);
        }
        m10 += msum; m01 += v * vs;
    }
    const float PI_F = 3.14159265f;
    float a = (float)atan2((double)(float)m01, (double)(float)m10);
    if (a < 0) a += 2.0f * PI_F;
    return a * (180.0f / PI_F);
}

// computeOrbDescriptor<2> (orb.cu:222-246, :352-367): byte b of keypoint p = 8 tests on the pattern rotated by the keypoint angle
__device__ __forceinline__ int orb_desc_byte(const uint8_t *__restrict__ img, size_t step, int x, int y, float angle, int b)
{
    const float PI_F = 3.14159265f;
    const float a = angle * (float)(PI_F / 180.f);
    const float sina = (float)sin((double)a), cosa = (float)cos((double)a);
    auto val = [&](int idx) {
        const float px = (float)c_pattern[16 * b + idx].x, py = (float)c_pattern[16 * b + idx].y;
        const int yy = y + (int)__builtin_rintf(px * sina + py * cosa), xx = x + (int)__builtin_rintf(px * cosa - py * sina);
        return (int)img[(size_t)yy * step + xx];
    };
    int v = 0;
#pragma unroll
    for (int t = 0; t < 8; ++t) v |= (val(2 * t) < val(2 * t + 1)) << t;
    return v;
}

// ---- RANSAC: per 4-point hypothesis HomographyEstimatorCallback::runKernel (fundam.cpp:80-142, k_ransac_fit: one lane a hypothesis), then the inlier count
// of RANSACPointSetRegistrator::findInliers with computeError's float arithmetic (fundam.cpp:144-166, ptsetreg.cpp:85-104; k_ransac_score)
// Every loop over matrix entries is unrolled in full, so that on the device the two 9 x 9 matrices live in registers under constant indices and not in scratch
// memory under computed ones; the operations and their order are untouched (no contraction, no reassociation: the same bits, host and device).
__host__ __device__ inline void jacobi_eig9(double A[9][9], double V[9][9], double w[9])
{
#pragma unroll
    for (int i = 0; i < 9; ++i) {
#pragma unroll
        for (int j = 0; j < 9; ++j) V[i][j] = 0;
        V[i][i] = 1;
    }
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
#pragma unroll
            for (int j = i + 1; j < 9; ++j) off += A[i][j] * A[i][j];
        }
        if (off < 1e-300) break;
#pragma unroll
        for (int p = 0; p < 8; ++p) {
#pragma unroll
            for (int q = p + 1; q < 9; ++q) {
                const double apq = A[p][q];
                if (fabs(apq) < 1e-300) continue;
                const double theta = (A[q][q] - A[p][p]) / (2 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1));
                const double c = 1 / sqrt(t * t + 1), s = t * c;
#pragma unroll
                for (int k = 0; k < 9; ++k) { const double akp = A[k][p], akq = A[k][q]; A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq; }
#pragma unroll
                for (int k = 0; k < 9; ++k) { const double apk = A[p][k], aqk = A[q][k]; A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk; }
#pragma unroll
                for (int k = 0; k < 9; ++k) { const double vkp = V[k][p], vkq = V[k][q]; V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq; }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) w[i] = A[i][i];
}
}  // namespace

// (host and device) the DLT of runKernel on `count` correspondences M[i] -> m[i]; false where the reference returns 0 models
__host__ __device__ static bool homography_dlt(const float *Mx, const float *My, const float *mx, const float *my, int count, double H[9])
{
    double cMx = 0, cMy = 0, cmx = 0, cmy = 0, sMx = 0, sMy = 0, smx = 0, smy = 0;
    for (int i = 0; i < count; ++i) { cmx += mx[i]; cmy += my[i]; cMx += Mx[i]; cMy += My[i]; }
    cmx /= count; cmy /= count; cMx /= count; cMy /= count;
    for (int i = 0; i < count; ++i) { smx += fabs(mx[i] - cmx); smy += fabs(my[i] - cmy); sMx += fabs(Mx[i] - cMx); sMy += fabs(My[i] - cMy); }
    if (fabs(smx) < DBL_EPSILON || fabs(smy) < DBL_EPSILON || fabs(sMx) < DBL_EPSILON || fabs(sMy) < DBL_EPSILON) return false;
    smx = count / smx; smy = count / smy; sMx = count / sMx; sMy = count / sMy;
    double L[9][9], V[9][9], w[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) {
#pragma unroll
        for (int k = 0; k < 9; ++k) L[j][k] = 0;
    }
    for (int i = 0; i < count; ++i) {
        const double x = (mx[i] - cmx) * smx, y = (my[i] - cmy) * smy, X = (Mx[i] - cMx) * sMx, Y = (My[i] - cMy) * sMy;
        const double Lx[9] = {X, Y, 1, 0, 0, 0, -x * X, -x * Y, -x}, Ly[9] = {0, 0, 0, X, Y, 1, -y * X, -y * Y, -y};
#pragma unroll
        for (int j = 0; j < 9; ++j) {
#pragma unroll
            for (int k = j; k < 9; ++k) L[j][k] += Lx[j] * Lx[k] + Ly[j] * Ly[k];
        }
    }
#pragma unroll
    for (int j = 0; j < 9; ++j) {
#pragma unroll
        for (int k = 0; k < j; ++k) L[j][k] = L[k][j];
    }
    jacobi_eig9(L, V, w);
    double wbest = w[0], h0[9];                                             // cv::eigen sorts descending and the reference takes the last row: the FIRST smallest
#pragma unroll
    for (int i = 0; i < 9; ++i) h0[i] = V[i][0];
#pragma unroll
    for (int c = 1; c < 9; ++c) {
        const bool lower = w[c] < wbest;
        wbest = lower ? w[c] : wbest;
#pragma unroll
        for (int i = 0; i < 9; ++i) h0[i] = lower ? V[i][c] : h0[i];
    }
    const double inv[9] = {1. / smx, 0, cmx, 0, 1. / smy, cmy, 0, 0, 1}, nrm[9] = {sMx, 0, -cMx * sMx, 0, sMy, -cMy * sMy, 0, 0, 1};
    double t[9];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) t[3 * r + c] = inv[3 * r] * h0[c] + inv[3 * r + 1] * h0[3 + c] + inv[3 * r + 2] * h0[6 + c];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) H[3 * r + c] = t[3 * r] * nrm[c] + t[3 * r + 1] * nrm[3 + c] + t[3 * r + 2] * nrm[6 + c];
    const double s = 1. / H[8];
    for (int i = 0; i < 9; ++i) H[i] *= s;
    return true;
}
// (host and device) computeError + the threshold compare of findInliers over the points [i0, i1): the model's first 8 entries as floats, every point
// the same float operations in the same order whoever calls it -- the score kernel on its wave's share of a chunk in LDS, the host for the winner's mask
__host__ __device__ static inline int homography_inliers_range(const float h[8], const float *Mx, const float *My, const float *mx, const float *my, int i0, int i1, float t,
                                                               uint8_t *mask)
{
    const float h0 = h[0], h1 = h[1], h2 = h[2], h3 = h[3], h4 = h[4], h5 = h[5], h6 = h[6], h7 = h[7];
    int good = 0;
    for (int i = i0; i < i1; ++i) {
        const float ww = 1.f / (h6 * Mx[i] + h7 * My[i] + 1.f);
        const float dx = (h0 * Mx[i] + h1 * My[i] + h2) * ww - mx[i], dy = (h3 * Mx[i] + h4 * My[i] + h5) * ww - my[i];
        const int f = dx * dx + dy * dy <= t;
        if (mask) mask[i] = (uint8_t)f;
        good += f;
    }
    return good;
}
__host__ __device__ static inline int homography_inliers(const double H[9], const float *Mx, const float *My, const float *mx, const float *my, int n, float t, uint8_t *mask)
{
    float h[8];
    for (int k = 0; k < 8; ++k) h[k] = (float)H[k];
    return homography_inliers_range(h, Mx, My, mx, my, 0, n, t, mask);
}

namespace {
// ---- batched RANSAC: the hypotheses of every problem of a batch in two launches.  The fit (a 9 x 9 double eigen-solve a lane) and the scoring (a float loop over
// the problem's points) are separate kernels: the fit's register and scratch state does not sit on the scoring loop, and the scoring spreads a problem's points
// over the waves of a workgroup instead of walking them all in one lane.
constexpr int RS_LANES = 64;                                    // hypotheses a score workgroup takes: one a lane, the same in each of its waves
constexpr int RS_WAVES = 4;                                     // waves of a score workgroup
constexpr int RS_WAVE_POINTS = 128;                             // W: the points one wave takes of a chunk
constexpr int RS_CHUNK = RS_WAVES * RS_WAVE_POINTS;             // C = 512: the points staged in LDS at a time (4 float planes: 8 KiB)
struct RsProb { int pt_off, n, hyp_off, n_hyp; };               // a problem's slice of the point planes and of the hypothesis arrays
struct RsBlock { int prob, hyp0; };                             // a score workgroup: hypotheses [hyp0, hyp0 + 64) of problem prob
struct RsHyp { int prob, i0, i1, i2, i3; };                     // a hypothesis: its problem and its four points (indices into the problem's slice)

// pts: four planes of n_pts floats (Mx, My, mx, my), every problem's points at its pt_off
__global__ void __launch_bounds__(64) k_ransac_fit(const float *__restrict__ pts, size_t n_pts, const RsProb *__restrict__ probs, const RsHyp *__restrict__ hyps, int n_hyp,
                                                   double *__restrict__ models, int *__restrict__ valid)
{
    const int g = blockIdx.x * 64 + threadIdx.x;
    if (g >= n_hyp) return;
    const RsHyp r = hyps[g];
    const float *Mx = pts + probs[r.prob].pt_off, *My = Mx + n_pts, *mx = My + n_pts, *my = mx + n_pts;
    const int idx[4] = {r.i0, r.i1, r.i2, r.i3};
    float sMx[4], sMy[4], smx[4], smy[4];
    for (int k = 0; k < 4; ++k) { const int i = idx[k]; sMx[k] = Mx[i]; sMy[k] = My[i]; smx[k] = mx[i]; smy[k] = my[i]; }
    double H[9];
    const bool ok = homography_dlt(sMx, sMy, smx, smy, 4, H);
    if (!ok) for (int i = 0; i < 9; ++i) H[i] = 0;
    valid[g] = ok ? 1 : 0;
    for (int i = 0; i < 9; ++i) models[9 * (size_t)g + i] = H[i];
}

// One workgroup per (problem, 64 hypotheses).  Lane l of EVERY wave holds hypothesis hyp0 + l; the problem's points pass through LDS in chunks of RS_CHUNK, and wave w
// counts the inliers among points [w * RS_WAVE_POINTS, (w + 1) * RS_WAVE_POINTS) of each chunk.  All lanes of a wave read the same LDS address (a broadcast, no bank
// conflict).  The counts are integers, so the split changes nothing; the waves' counts are added through LDS at the end.  good = -1: the hypothesis has no model.
__global__ void __launch_bounds__(RS_LANES * RS_WAVES) k_ransac_score(const float *__restrict__ pts, size_t n_pts, const RsProb *__restrict__ probs,
                                                                       const RsBlock *__restrict__ blocks, const double *__restrict__ models,
                                                                       const int *__restrict__ valid, float thresh_sq, int *__restrict__ good)
{
    __shared__ float s_pts[4][RS_CHUNK];
    __shared__ int s_cnt[RS_WAVES][RS_LANES];
    const RsBlock b = blocks[blockIdx.x];
    const RsProb p = probs[b.prob];
    const int lane = threadIdx.x & (RS_LANES - 1), wave = threadIdx.x / RS_LANES;
    const bool live = b.hyp0 + lane < p.n_hyp;
    const size_t g = (size_t)p.hyp_off + (size_t)(b.hyp0 + lane);
    const bool has = live && valid[g] != 0;
    float h[8];
    for (int k = 0; k < 8; ++k) h[k] = has ? (float)models[9 * g + k] : 0.f;
    int cnt = 0;
    for (int c0 = 0; c0 < p.n; c0 += RS_CHUNK) {
        const int m = min(RS_CHUNK, p.n - c0);
        __syncthreads();                                        // the chunk before is counted
        for (int i = threadIdx.x; i < m; i += RS_LANES * RS_WAVES)
            for (int pl = 0; pl < 4; ++pl) s_pts[pl][i] = pts[pl * n_pts + (size_t)(p.pt_off + c0 + i)];
        __syncthreads();
        const int i0 = wave * RS_WAVE_POINTS, i1 = min(m, i0 + RS_WAVE_POINTS);
        if (has && i0 < i1) cnt += homography_inliers_range(h, s_pts[0], s_pts[1], s_pts[2], s_pts[3], i0, i1, thresh_sq, nullptr);
    }
    s_cnt[wave][lane] = cnt;
    __syncthreads();
    if (wave == 0 && live) {
        int sum = 0;
        for (int w = 0; w < RS_WAVES; ++w) sum += s_cnt[w][lane];
        good[g] = has ? sum : -1;
    }
}

// the winners' models out of the model array: 9 doubles per listed hypothesis
__global__ void __launch_bounds__(64) k_ransac_gather(const double *__restrict__ models, const int *__restrict__ win, int n_win, double *__restrict__ out)
{
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t < 9 * n_win) out[t] = models[9 * (size_t)win[t / 9] + t % 9];
}

// cv::RNG (core/include/opencv2/core/operations.hpp: multiply-with-carry, CV_RNG_COEFF 4164903690)
struct CvRng {
    unsigned long long state;
    explicit CvRng(unsigned long long s) : state(s ? s : 0xffffffffull) {}
    unsigned next() { state = (unsigned long long)(unsigned)state * 4164903690ull + (unsigned)(state >> 32); return (unsigned)state; }
    int uniform(int a, int b) { return a == b ? a : (int)(next() % (unsigned)(b - a) + a); }
};

bool collinear_last(const float *x, const float *y, int count)            // haveCollinearPoints (calib3d/src/precomp.hpp:118-139): only the LAST point is tested
{
    const int i = count - 1;
    for (int j = 0; j < i; ++j) {
        const double dx1 = x[j] - x[i], dy1 = y[j] - y[i];
        for (int k = 0; k < j; ++k) {
            const double dx2 = x[k] - x[i], dy2 = y[k] - y[i];
            if (std::fabs(dx2 * dy1 - dy2 * dx1) <= FLT_EPSILON * (std::fabs(dx1) + std::fabs(dy1) + std::fabs(dx2) + std::fabs(dy2))) return true;
        }
    }
    return false;
}
bool check_subset4(const float *sx, const float *sy, const float *dx, const float *dy)      // HomographyEstimatorCallback::checkSubset (fundam.cpp:49-78)
{
    if (collinear_last(sx, sy, 4) || collinear_last(dx, dy, 4)) return false;
    static const int tt[4][3] = {{0, 1, 2}, {1, 2, 3}, {0, 2, 3}, {0, 1, 3}};
    int negative = 0;
    for (int i = 0; i < 4; ++i) {
        const int *t = tt[i];
        auto det = [&](const float *x, const float *y) {
            const double a = x[t[0]], b = y[t[0]], c = x[t[1]], d = y[t[1]], e = x[t[2]], f = y[t[2]];
            return a * (d - f) - b * (c - e) + (c * f - d * e);            // Matx33d determinant, rows (x, y, 1)
        };
        negative += det(sx, sy) * det(dx, dy) < 0;
    }
    return negative == 0 || negative == 4;
}

int ransac_update_iters(double p, double ep, int model_points, int max_iters)       // RANSACUpdateNumIters (ptsetreg.cpp:53-73)
{
    p = std::min(std::max(p, 0.), 1.); ep = std::min(std::max(ep, 0.), 1.);
    double num = std::max(1. - p, DBL_MIN), denom = 1. - std::pow(1. - ep, model_points);
    if (denom < DBL_MIN) return 0;
    num = std::log(num); denom = std::log(denom);
    return denom >= 0 || -num >= max_iters * (-denom) ? max_iters : (int)std::nearbyint(num / denom);
}

// solve the 8 x 8 symmetric system (A + lambda diag) d = v by Gaussian elimination with partial pivoting (the reference: solve(..., DECOMP_EIG))
bool solve8(const double A[8][8], const double v[8], double d[8])
{
    double M[8][9];
    for (int i = 0; i < 8; ++i) { for (int j = 0; j < 8; ++j) M[i][j] = A[i][j]; M[i][8] = v[i]; }
    for (int i = 0; i < 8; ++i) {
        int p = i;
        for (int r = i + 1; r < 8; ++r) if (std::fabs(M[r][i]) > std::fabs(M[p][i])) p = r;
        if (std::fabs(M[p][i]) < 1e-300) return false;
        if (p != i) for (int c = 0; c < 9; ++c) std::swap(M[i][c], M[p][c]);
        for (int r = i + 1; r < 8; ++r) { const double f = M[r][i] / M[i][i]; for (int c = i; c < 9; ++c) M[r][c] -= f * M[i][c]; }
    }
    for (int i = 7; i >= 0; --i) { double s = M[i][8]; for (int c = i + 1; c < 8; ++c) s -= M[i][c] * d[c]; d[i] = s / M[i][i]; }
    return true;
}

// HomographyRefineCallback::compute (fundam.cpp:175-214) + LMSolverImpl::run, 10 iterations (levmarq.cpp:88-199)
void lm_refine(const float *Mx, const float *My, const float *mx, const float *my, int count, double h[8])
{
    auto compute = [&](const double *p, std::vector<double> &err, double (*JtJ)[8], double *Jtr) {
        err.resize(2 * (size_t)count);
        if (JtJ) { for (int a = 0; a < 8; ++a) { for (int b = 0; b < 8; ++b) JtJ[a][b] = 0; Jtr[a] = 0; } }
        for (int i = 0; i < count; ++i) {
            const double X = Mx[i], Y = My[i];
            double ww = p[6] * X + p[7] * Y + 1.;
            ww = std::fabs(ww) > DBL_EPSILON ? 1. / ww : 0;
            const double xi = (p[0] * X + p[1] * Y + p[2]) * ww, yi = (p[3] * X + p[4] * Y + p[5]) * ww;
            err[2 * i] = xi - mx[i]; err[2 * i + 1] = yi - my[i];
            if (JtJ) {
                const double J0[8] = {X * ww, Y * ww, ww, 0, 0, 0, -X * ww * xi, -Y * ww * xi}, J1[8] = {0, 0, 0, X * ww, Y * ww, ww, -X * ww * yi, -Y * ww * yi};
                for (int a = 0; a < 8; ++a) {
                    for (int b = 0; b < 8; ++b) JtJ[a][b] += J0[a] * J0[b] + J1[a] * J1[b];
                    Jtr[a] += J0[a] * err[2 * i] + J1[a] * err[2 * i + 1];
                }
            }
        }
    };
    auto sq = [](const std::vector<double> &e) { double s = 0; for (double v : e) s += v * v; return s; };
    double x[8], xd[8], A[8][8], v[8], D[8], d[8];
    memcpy(x, h, sizeof(x));
    std::vector<double> r, rd;
    compute(x, r, A, v);
    double S = sq(r);
    for (int i = 0; i < 8; ++i) D[i] = A[i][i];
    const double Rlo = 0.25, Rhi = 0.75;
    double lambda = 1, lc = 0.75;
    for (int iter = 0;;) {
        double Ap[8][8];
        memcpy(Ap, A, sizeof(Ap));
        for (int i = 0; i < 8; ++i) Ap[i][i] += lambda * D[i];
        if (!solve8(Ap, v, d)) break;
        for (int i = 0; i < 8; ++i) xd[i] = x[i] - d[i];
        compute(xd, rd, nullptr, nullptr);
        const double Sd = sq(rd);
        double dS = 0, dv = 0;
        for (int i = 0; i < 8; ++i) { double t = 2 * v[i]; for (int j = 0; j < 8; ++j) t -= A[i][j] * d[j]; dS += d[i] * t; dv += d[i] * v[i]; }
        const double R = (S - Sd) / (std::fabs(dS) > DBL_EPSILON ? dS : 1);
        if (R > Rhi) { lambda *= 0.5; if (lambda < lc) lambda = 0; }
        else if (R < Rlo) {
            double nu = (Sd - S) / (std::fabs(dv) > DBL_EPSILON ? dv : 1) + 2;
            nu = std::min(std::max(nu, 2.), 10.);
            if (lambda == 0) {
                double maxval = DBL_EPSILON;              // largest diagonal entry of inv(A): one unit-vector solve per column
                for (int c = 0; c < 8; ++c) { double e[8] = {0}, col[8]; e[c] = 1; if (solve8(A, e, col)) maxval = std::max(maxval, std::fabs(col[c])); }
                lambda = lc = 1. / maxval;
                nu *= 0.5;
            }
            lambda *= nu;
        }
        if (Sd < S) { S = Sd; memcpy(x, xd, sizeof(x)); compute(x, r, A, v); }
        ++iter;
        double nd = 0, nr = 0;
        for (int i = 0; i < 8; ++i) nd = std::max(nd, std::fabs(d[i]));
        for (double e : r) nr = std::max(nr, std::fabs(e));
        if (!(iter < 10 && nd >= FLT_EPSILON && nr >= FLT_EPSILON)) break;
    }
    memcpy(h, x, sizeof(x));
}

static inline size_t rs_align(size_t n) { return (n + 255) & ~(size_t)255; }

// One problem of a batch on the host: its points as planes, what the device is asked about it and what comes back
struct RsProblem {
    int n = 0;
    std::vector<float> Mx, My, mx, my;
    std::vector<uint8_t> mask;
    double H[9] = {0};
    bool ok = false;
    int dev = -1;                   // index among the problems that go to the device, -1: settled on the host
    int drawn = 0;                  // hypotheses drawn
    size_t sub_off = 0;             // its first hypothesis in the batch's subset list
};

// cv::findHomography(RANSAC) on every problem of a batch; the arguments are checked and a device is present.  Per problem the steps of the reference in their order;
// the device work of ALL problems goes out in one pass: 1 upload, k_ransac_fit, k_ransac_score, 1 copy back (the counts), 1 synchronise; then the sequential scans
// on the host and, where a problem has a winner, 1 upload (the winners' hypothesis numbers), k_ransac_gather, 1 copy back (their models), 1 synchronise:
// 3 launches, 4 copies, 2 synchronisations at most, whatever n_problems is; none where no problem reaches the device.
int ransac_batch(const char *fn, int n_problems, const int *offsets, const float *src_xy, const float *dst_xy, double reproj_threshold, int max_iters, double confidence,
                 double *H_out, uint8_t *inlier_mask, int *n_inliers, int *status, ms_stream stream)
{
    if (reproj_threshold <= 0) reproj_threshold = 3;                       // defaultRANSACReprojThreshold (fundam.cpp:325, :351)
    if (max_iters <= 0) max_iters = 2000;
    if (!(confidence > 0 && confidence < 1)) confidence = 0.995;
    const float t = (float)(reproj_threshold * reproj_threshold);
    const int total_pts = offsets[n_problems];
    for (int p = 0; p < n_problems; ++p) { status[p] = 1; if (n_inliers) n_inliers[p] = 0; }
    for (size_t i = 0; i < 9 * (size_t)n_problems; ++i) H_out[i] = 0;
    if (inlier_mask && total_pts > 0) memset(inlier_mask, 0, (size_t)total_pts);

    std::vector<RsProblem> P(n_problems);
    std::vector<int> subsets;                                              // 4 point indices per hypothesis, the device problems one after another
    int n_dev = 0;
    size_t dev_pts = 0, n_blocks = 0;
    for (int p = 0; p < n_problems; ++p) {
        RsProblem &q = P[p];
        const int n = q.n = offsets[p + 1] - offsets[p];
        if (n < 4) continue;                                               // (the reference returns an empty Mat)
        const float *s = src_xy + 2 * (size_t)offsets[p], *d = dst_xy + 2 * (size_t)offsets[p];
        q.Mx.resize(n); q.My.resize(n); q.mx.resize(n); q.my.resize(n); q.mask.assign(n, 0);
        for (int i = 0; i < n; ++i) { q.Mx[i] = s[2 * i]; q.My[i] = s[2 * i + 1]; q.mx[i] = d[2 * i]; q.my[i] = d[2 * i + 1]; }
        if (n == 4) {                                                      // method == 0 || npoints == 4 (fundam.cpp:356-360)
            q.ok = homography_dlt(q.Mx.data(), q.My.data(), q.mx.data(), q.my.data(), 4, q.H);
            std::fill(q.mask.begin(), q.mask.end(), (uint8_t)1);
            continue;
        }
        // every subset the sequential loop COULD draw, in its order (ptsetreg.cpp:106-173): the draw does not depend on the models found
        CvRng rng((unsigned long long)-1);
        q.sub_off = subsets.size() / 4;
        int drawn = 0;
        for (; drawn < max_iters; ++drawn) {
            int idx[4];
            bool found = false;
            for (int iters = 0; iters < 10000; ++iters) {
                for (int i = 0; i < 4; ++i) {
                    for (;;) { idx[i] = rng.uniform(0, n); int j = 0; for (; j < i; ++j) if (idx[i] == idx[j]) break; if (j == i) break; }
                }
                float sx[4], sy[4], dx[4], dy[4];
                for (int i = 0; i < 4; ++i) { sx[i] = q.Mx[idx[i]]; sy[i] = q.My[idx[i]]; dx[i] = q.mx[idx[i]]; dy[i] = q.my[idx[i]]; }
                if (check_subset4(sx, sy, dx, dy)) { found = true; break; }
            }
            if (!found) break;
            subsets.insert(subsets.end(), idx, idx + 4);
        }
        if (drawn == 0) continue;
        q.drawn = drawn; q.dev = n_dev++;
        dev_pts += (size_t)n;
        n_blocks += (size_t)div_up(drawn, RS_LANES);
    }

    if (n_dev) {
        const size_t n_hyp = subsets.size() / 4;
        if (n_hyp > (size_t)INT_MAX / 16 || dev_pts > (size_t)INT_MAX / 16)
            return fail(MS_ERR_INVALID, "%s: %zu hypotheses over %zu points are more than one batch holds", fn, n_hyp, dev_pts);
        hipStream_t st = as_stream(stream);
        // the upload, packed: point planes, problems, score workgroups, hypotheses; behind it on the device the models, flags and counts, the winners' list and models
        const size_t o_pts = 0, o_probs = o_pts + rs_align(4 * dev_pts * sizeof(float)), o_blocks = o_probs + rs_align((size_t)n_dev * sizeof(RsProb)),
                     o_hyps = o_blocks + rs_align(n_blocks * sizeof(RsBlock)), up_bytes = o_hyps + rs_align(n_hyp * sizeof(RsHyp));
        const size_t o_models = up_bytes, o_valid = o_models + rs_align(9 * n_hyp * sizeof(double)), o_good = o_valid + rs_align(n_hyp * sizeof(int)),
                     o_win = o_good + rs_align(n_hyp * sizeof(int)), o_winH = o_win + rs_align((size_t)n_dev * sizeof(int)),
                     dev_bytes = o_winH + rs_align(9 * (size_t)n_dev * sizeof(double));
        const size_t h_good = up_bytes, h_win = h_good + rs_align(n_hyp * sizeof(int)), h_winH = h_win + rs_align((size_t)n_dev * sizeof(int)),
                     pin_bytes = h_winH + rs_align(9 * (size_t)n_dev * sizeof(double));
        char *dev = (char *)device_scratch().get(dev_bytes);                // per-thread grow-only block: see DeviceScratch (common.hpp)
        if (!dev) return fail(MS_ERR_NOMEM, "%s: cannot allocate %zu bytes of device scratch", fn, dev_bytes);
        char *pin = (char *)pinned_scratch().get(pin_bytes);
        if (!pin) return fail(MS_ERR_NOMEM, "%s: cannot allocate pinned staging memory", fn);
        float *hp = (float *)(pin + o_pts);
        RsProb *hprob = (RsProb *)(pin + o_probs);
        RsBlock *hblk = (RsBlock *)(pin + o_blocks);
        RsHyp *hhyp = (RsHyp *)(pin + o_hyps);
        size_t pt = 0, blk = 0;
        for (int p = 0; p < n_problems; ++p) {
            const RsProblem &q = P[p];
            if (q.dev < 0) continue;
            memcpy(hp + pt, q.Mx.data(), sizeof(float) * q.n); memcpy(hp + dev_pts + pt, q.My.data(), sizeof(float) * q.n);
            memcpy(hp + 2 * dev_pts + pt, q.mx.data(), sizeof(float) * q.n); memcpy(hp + 3 * dev_pts + pt, q.my.data(), sizeof(float) * q.n);
            hprob[q.dev] = RsProb{(int)pt, q.n, (int)q.sub_off, q.drawn};
            for (int h0 = 0; h0 < q.drawn; h0 += RS_LANES) hblk[blk++] = RsBlock{q.dev, h0};
            for (int h = 0; h < q.drawn; ++h) {
                const int *s = &subsets[4 * (q.sub_off + h)];
                hhyp[q.sub_off + h] = RsHyp{q.dev, s[0], s[1], s[2], s[3]};
            }
            pt += (size_t)q.n;
        }
        const float *d_pts = (const float *)(dev + o_pts);
        const RsProb *d_probs = (const RsProb *)(dev + o_probs);
        double *d_models = (double *)(dev + o_models);
        int *d_valid = (int *)(dev + o_valid), *d_good = (int *)(dev + o_good);
        hipError_t e = hipMemcpyAsync(dev, pin, up_bytes, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) {
            k_ransac_fit<<<(unsigned)div_up((int)n_hyp, 64), 64, 0, st>>>(d_pts, dev_pts, d_probs, (const RsHyp *)(dev + o_hyps), (int)n_hyp, d_models, d_valid);
            e = hipGetLastError();
        }
        if (e == hipSuccess) {
            k_ransac_score<<<(unsigned)n_blocks, RS_LANES * RS_WAVES, 0, st>>>(d_pts, dev_pts, d_probs, (const RsBlock *)(dev + o_blocks), d_models, d_valid, t, d_good);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(pin + h_good, d_good, n_hyp * sizeof(int), hipMemcpyDeviceToHost, st);
        hipError_t se = hipStreamSynchronize(st);          // also after a failed enqueue: nothing of this call stays in flight over the scratch blocks
        MS_HIP(e);
        MS_HIP(se);
        // the sequential scan of RANSACPointSetRegistrator::run (ptsetreg.cpp:208-240) per problem: first strictly better model wins, the iteration budget shrinks as it goes
        const int *good = (const int *)(pin + h_good);
        int *win = (int *)(pin + h_win);
        std::vector<int> win_prob;
        for (int p = 0; p < n_problems; ++p) {
            const RsProblem &q = P[p];
            if (q.dev < 0) continue;
            const int *g = good + q.sub_off;
            int niters = std::max(max_iters, 1), max_good = 0, best = -1;
            for (int iter = 0; iter < niters && iter < q.drawn; ++iter) {
                if (g[iter] < 0) continue;                                 // runKernel returned no model
                if (g[iter] > q.n) return fail(MS_ERR_HIP, "%s: the device returned an impossible inlier count (%d of %d points)", fn, g[iter], q.n);
                if (g[iter] > std::max(max_good, 3)) {
                    best = iter; max_good = g[iter];
                    niters = ransac_update_iters(confidence, (double)(q.n - max_good) / q.n, 4, niters);
                }
            }
            if (best >= 0) { win[win_prob.size()] = (int)(q.sub_off + best); win_prob.push_back(p); }
        }
        if (!win_prob.empty()) {
            const int n_win = (int)win_prob.size();
            e = hipMemcpyAsync(dev + o_win, pin + h_win, (size_t)n_win * sizeof(int), hipMemcpyHostToDevice, st);
            if (e == hipSuccess) {
                k_ransac_gather<<<(unsigned)div_up(9 * n_win, 64), 64, 0, st>>>(d_models, (const int *)(dev + o_win), n_win, (double *)(dev + o_winH));
                e = hipGetLastError();
            }
            if (e == hipSuccess) e = hipMemcpyAsync(pin + h_winH, dev + o_winH, 9 * (size_t)n_win * sizeof(double), hipMemcpyDeviceToHost, st);
            se = hipStreamSynchronize(st);
            MS_HIP(e);
            MS_HIP(se);
            for (int k = 0; k < n_win; ++k) {
                RsProblem &q = P[win_prob[k]];
                memcpy(q.H, pin + h_winH + 72 * (size_t)k, sizeof(q.H));
                homography_inliers(q.H, q.Mx.data(), q.My.data(), q.mx.data(), q.my.data(), q.n, t, q.mask.data());
                q.ok = true;
            }
        }
    }

    std::vector<float> iMx, iMy, imx, imy;
    for (int p = 0; p < n_problems; ++p) {
        RsProblem &q = P[p];
        if (!q.ok) continue;
        const int n = q.n;
        // compressElems + runKernel on the inliers + Levenberg-Marquardt polish (fundam.cpp:370-385)
        if (n > 4) {
            iMx.clear(); iMy.clear(); imx.clear(); imy.clear();
            for (int i = 0; i < n; ++i) if (q.mask[i]) { iMx.push_back(q.Mx[i]); iMy.push_back(q.My[i]); imx.push_back(q.mx[i]); imy.push_back(q.my[i]); }
            const int m = (int)iMx.size();
            if (m > 0) {
                double H2[9];
                if (homography_dlt(iMx.data(), iMy.data(), imx.data(), imy.data(), m, H2)) memcpy(q.H, H2, sizeof(q.H));
                lm_refine(iMx.data(), iMy.data(), imx.data(), imy.data(), m, q.H);      // the 8 free parameters; H[8] stays 1
            }
        }
        memcpy(H_out + 9 * (size_t)p, q.H, sizeof(q.H));
        int cnt = 0;
        uint8_t *mk = inlier_mask ? inlier_mask + offsets[p] : nullptr;
        for (int i = 0; i < n; ++i) { if (mk) mk[i] = q.mask[i]; cnt += q.mask[i]; }
        if (n_inliers) n_inliers[p] = cnt;
        status[p] = 0;
    }
    return MS_OK;
}

// ---- ORB: cuda::ORB::detectAndCompute (orb.cpp:430-865) for every view of a rig in one device pass, no host in the loop.
// A SEGMENT is one pyramid level of one view.  Everything the reference's host code decides per level -- sizes (orb.cpp:668), budgets (:501-512), the detector's
// buffer (:753), where the level's image, mask and score map live -- follows from the shapes and the parameters alone and goes up once, as a table; what depends on
// the pixels (the counts between the stages) stays on the device.  Every kernel is launched once for all segments: a workgroup finds its segment in a list of
// (first work item, segment) by bisection.
constexpr int OB_MAX_SEG = MS_MAX_VIEWS * 16;
constexpr int OB_SORT_TILE = 1024;                              // Harris keys staged in LDS at a time (4 KiB)
struct ObSeg {
    const uint8_t *img, *mask;                                  // level 0: the caller's image and mask as they are; above: in the arena.  mask null: none
    uint8_t *score;                                             // FAST score map of the level (step w); null where the budget is <= 0
    uint8_t *desc;                                              // the view's descriptor matrix
    size_t step, mstep, dstep;
    int w, h, view, level, first;                               // first: the view's level-0 segment (its segments follow one another)
    int n, max_npoints;                                         // the level's budget (orb.cpp:501-512) and the detector's buffer (orb.cpp:753)
    int cap_b, cap_c;                                           // rows the level can hold after the first and the second cull: min(max_npoints, 2n), min(max_npoints, n)
    int row_off, a_off, b_off, c_off;                           // its slices of the row arrays and of the three candidate arrays
    float ifx, ify;                                             // resize from the level below: static_cast<float>(1.0 / fx) of launch_resize_linear
    float loc_scale, size;                                      // mergeKeyPoints' factors (orb.cpp:823-865)
};
template <int N> struct ObList { int n, total; int start[N + 1], seg[N]; };         // segment seg[k] owns the work items start[k] .. start[k + 1] - 1
struct ObTable {
    int umax[32];
    ObSeg segs[OB_MAX_SEG];
    ObList<MS_MAX_VIEWS> pyr[16];                               // the 64 x 4 tiles of level l >= 1 of every view that has one
    ObList<OB_MAX_SEG> tiles, rows, active, harris, sort, finish, desc; // tiles and rows of the scored segments; those segments; blocks of 64 / 256 / 64 / 8 keypoints
};
struct ObBufs {
    int *rowraw, *rowcnt;                                       // per row of every scored segment: raw corners, survivors (counts, then exclusive offsets inside the segment)
    int *cnt_a, *cnt_b, *cnt_c;                                 // per segment: candidates after suppression, after the first cull, after the second
    short2 *loc_a, *loc_b, *loc_c;
    uint8_t *score_a;                                           // FAST response of the candidates (1..255)
    float *resp_b, *resp_c;                                     // Harris responses
    float *kp;                                                  // n_views x max_keypoints x 6
    int max_keypoints, half;                                    // half: patch_size / 2
};

template <int N> __device__ __forceinline__ int ob_find(const ObList<N> &L, int item, int &local)
{
    int lo = 0, hi = L.n;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (L.start[mid] <= item) lo = mid; else hi = mid; }
    local = item - L.start[lo];
    return L.seg[lo];
}

// k_resize_linear<1> (prims.hip; resize.cu:71-106) at one pixel: the same float operations in the same order
__device__ __forceinline__ uint8_t ob_resize_at(const uint8_t *__restrict__ src, size_t sstep, int srows, int scols, float ify, float ifx, int x, int y)
{
    const float sx = (float)x * ifx, sy = (float)y * ify;
    const int x1 = f2i_rd(sx), y1 = f2i_rd(sy);
    const int x2 = x1 + 1, y2 = y1 + 1;
    const int x2r = min(x2, scols - 1), y2r = min(y2, srows - 1);
    const float w11 = ((float)x2 - sx) * ((float)y2 - sy), w12 = (sx - (float)x1) * ((float)y2 - sy);
    const float w21 = ((float)x2 - sx) * (sy - (float)y1), w22 = (sx - (float)x1) * (sy - (float)y1);
    const uint8_t *r1 = row_ptr<uint8_t>(src, sstep, y1), *r2 = row_ptr<uint8_t>(src, sstep, y2r);
    float out = 0.f;
    out = __builtin_fmaf((float)r1[x1], w11, out);
    out = __builtin_fmaf((float)r1[x2r], w12, out);
    out = __builtin_fmaf((float)r2[x1], w21, out);
    out = __builtin_fmaf((float)r2[x2r], w22, out);
    return sat_u8(out);
}
// a. level l of every view from its level l - 1 (orb.cpp:686), the mask with it and through THRESH_TOZERO 254 (:690-693).  Equal sizes: the weights are 1, 0, 0, 0 -- a copy
__global__ void __launch_bounds__(256) k_ob_pyramid(const ObTable *__restrict__ T, int level)
{
    int tile;
    const ObSeg &s = T->segs[ob_find(T->pyr[level], blockIdx.x, tile)], &below = (&s)[-1];
    const int tiles_x = (s.w + 63) / 64, x = (tile % tiles_x) * 64 + threadIdx.x, y = (tile / tiles_x) * 4 + threadIdx.y;
    if (x >= s.w || y >= s.h) return;
    const_cast<uint8_t *>(s.img)[(size_t)y * s.step + x] = ob_resize_at(below.img, below.step, below.h, below.w, s.ify, s.ifx, x, y);
    if (s.mask) {
        const uint8_t m = ob_resize_at(below.mask, below.mstep, below.h, below.w, s.ify, s.ifx, x, y);
        const_cast<uint8_t *>(s.mask)[(size_t)y * s.mstep + x] = m <= 254 ? 0 : m;
    }
}
// b. the FAST score map (calcKeypoints<true>, fast.cu:264-307; 0 = no corner) of every scored segment, a 64 x 4 tile a workgroup.  The level's mask is the user's
// mask AND the inner rectangle left by edgeThreshold (orb.cpp:707-712)
__global__ void __launch_bounds__(256) k_ob_fast(const ObTable *__restrict__ T, int edge, int th)
{
    int tile;
    const ObSeg &s = T->segs[ob_find(T->tiles, blockIdx.x, tile)];
    const int tiles_x = (s.w + 63) / 64, j = (tile % tiles_x) * 64 + threadIdx.x, i = (tile / tiles_x) * 4 + threadIdx.y;
    if (j >= s.w || i >= s.h) return;
    s.score[(size_t)i * s.w + j] = (uint8_t)fast_score_at(s.img, s.step, s.h, s.w, s.mask, s.mstep, edge, th, i, j);
}
// c. suppression (nonmaxSuppression, fast.cu:346-371) and compaction in raster order instead of the reference's atomic order, one wave a row (4 rows a workgroup);
// a ballot gives the order inside a row.  One rule for every segment: the raw corners (score != 0, rows 3 .. h - 4, columns 3 .. w - 4) are numbered in raster
// order, those numbered below max_npoints (the detector's buffer, orb.cpp:753) are candidates, and a candidate survives when it is a strict maximum of its 8
// neighbours in the WHOLE score map.  Within the buffer every raw corner is a candidate.  Past it the reference keeps whichever max_npoints win its atomic
// counter (fast.cu:338-341); here the first ones in raster order do.
// PASS 0: raw corners of the row.  (scan.)  PASS 1: survivors of the row, from the raw offsets.  (scan.)  PASS 2: write them at the survivor offsets.
template <int PASS>
__global__ void __launch_bounds__(256) k_ob_rows(const ObTable *__restrict__ T, ObBufs B)
{
    const int item = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (item >= T->rows.total) return;
    int i;
    const ObSeg &s = T->segs[ob_find(T->rows, item, i)];
    const int row = s.row_off + i;
    const bool inner = i >= 3 && i < s.h - 3;
    const unsigned long long below = (1ull << lane) - 1ull;
    int raw = PASS == 0 ? 0 : B.rowraw[row], cnt = PASS == 2 ? B.rowcnt[row] : 0;
    if (inner)
        for (int j0 = 3; j0 < s.w - 3 && (PASS == 0 || raw < s.max_npoints); j0 += 64) {
            const int j = j0 + lane;
            const bool nz = j < s.w - 3 && s.score[(size_t)i * s.w + j] != 0;
            const unsigned long long mnz = __ballot(nz);
            if (PASS != 0) {
                const bool keep = nz && raw + __popcll(mnz & below) < s.max_npoints && is_local_max(s.score, (size_t)s.w, i, j);
                const unsigned long long mk = __ballot(keep);
                const int k = cnt + __popcll(mk & below);
                if (PASS == 2 && keep && k < s.max_npoints) { B.loc_a[s.a_off + k] = make_short2((short)j, (short)i); B.score_a[s.a_off + k] = s.score[(size_t)i * s.w + j]; }
                cnt += __popcll(mk);
            }
            raw += __popcll(mnz);
        }
    if (lane == 0) { if (PASS == 0) B.rowraw[row] = raw; if (PASS == 1) B.rowcnt[row] = cnt; }
}
// one segment a workgroup: exclusive scan of its rows in place (a lane sums a stretch of rows, then offsets them), the total to total[segment] when asked for
__global__ void __launch_bounds__(256) k_ob_scan(const ObTable *__restrict__ T, int *__restrict__ rows, int *__restrict__ total)
{
    __shared__ int s_part[256];
    const int sg = T->active.seg[blockIdx.x];
    const ObSeg &s = T->segs[sg];
    int *r = rows + s.row_off;
    const int per = (s.h + 255) / 256, a = threadIdx.x * per, b = min(a + per, s.h);
    int sum = 0;
    for (int i = a; i < b; ++i) sum += r[i];
    s_part[threadIdx.x] = sum;
    __syncthreads();
    int off = 0;
    for (int t = 0; t < (int)threadIdx.x; ++t) off += s_part[t];
    for (int i = a; i < b; ++i) { const int c = r[i]; r[i] = off; off += c; }
    if (threadIdx.x == 255 && total) total[sg] = off;
}
// d. cull to 2n by FAST response (orb.cpp:772; cull: :719-733, stable where thrust's device sort is not): untouched, in raster order, when the level holds no more; else the first 2n of the stable descending order, in that
// order.  The keys are 1..255.  One workgroup of 16 waves a segment; wave w owns the w-th sixteenth of the candidates (a stretch of the raster order).  A histogram
// per wave gives, summed, the threshold score t, the number q still wanted AT t and every score's first output row, and, scanned over the waves, how many of each
// score lie before a wave's stretch.  Then every wave walks its stretch 64 at a time: an element's place among its score is the count before the stretch + the
// count the wave has seen (a running count per score, score v in lane v % 64's register v / 64) + its rank among the equal lanes of the 64 (ballots, one score at
// a time); its row is its score's first row + that place; elements at t from place q on are dropped.  Counts come from atomics, the order never does.
constexpr int OB_CULL_WAVES = 16;
__global__ void __launch_bounds__(64 * OB_CULL_WAVES) k_ob_cull_fast(const ObTable *__restrict__ T, ObBufs B)
{
    __shared__ int s_hist[OB_CULL_WAVES][256], s_first[256], s_tq[2];
    const int sg = T->active.seg[blockIdx.x], tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const ObSeg &s = T->segs[sg];
    const int c = min(B.cnt_a[sg], s.max_npoints), keep = s.cap_b;
    const short2 *la = B.loc_a + s.a_off;
    const uint8_t *sa = B.score_a + s.a_off;
    short2 *lb = B.loc_b + s.b_off;
    if (c <= keep) {
        for (int i = tid; i < c; i += 64 * OB_CULL_WAVES) lb[i] = la[i];
        if (tid == 0) B.cnt_b[sg] = c;
        return;
    }
    const int per = (c + OB_CULL_WAVES - 1) / OB_CULL_WAVES, a = wave * per, b = min(a + per, c);
    for (int k = tid; k < OB_CULL_WAVES * 256; k += 64 * OB_CULL_WAVES) (&s_hist[0][0])[k] = 0;
    __syncthreads();
    for (int i = a + lane; i < b; i += 64) atomicAdd(&s_hist[wave][sa[i]], 1);
    __syncthreads();
    if (tid < 256) {                                            // per score: the counts before each wave's stretch, and the total
        int run = 0;
        for (int w = 0; w < OB_CULL_WAVES; ++w) { const int h = s_hist[w][tid]; s_hist[w][tid] = run; run += h; }
        s_first[tid] = run;
    }
    __syncthreads();
    if (tid == 0) {
        int acc = 0, t = 0, q = 0;
        for (int v = 255; v >= 1; --v) {
            const int total = s_first[v];
            s_first[v] = acc;
            if (!t && acc + total >= keep) { t = v; q = keep - acc; }
            acc += total;
        }
        s_tq[0] = t; s_tq[1] = q;
    }
    __syncthreads();
    const int t = s_tq[0], q = s_tq[1];
    const unsigned long long below = (1ull << lane) - 1ull;
    int seen[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) seen[k] = s_hist[wave][64 * k + lane];
    for (int base = a; base < b; base += 64) {
        const int i = base + lane, v = i < b ? (int)sa[i] : 0;
        const bool in = v >= t;
        unsigned long long todo = __ballot(in);
        int r = 0;
        while (todo) {                                          // the lanes of one score at a time
            const int lv = __builtin_amdgcn_readfirstlane(__shfl(v, __ffsll((long long)todo) - 1));
            const unsigned long long m = __ballot(in && v == lv);
            const int held = (lv >> 6) == 0 ? seen[0] : (lv >> 6) == 1 ? seen[1] : (lv >> 6) == 2 ? seen[2] : seen[3];
            const int before = __shfl(held, lv & 63);
            if (in && v == lv) r = before + __popcll(m & below);
#pragma unroll
            for (int k = 0; k < 4; ++k) seen[k] += (lane == (lv & 63) && k == (lv >> 6)) ? __popcll(m) : 0;
            todo &= ~m;
        }
        if (in && (v > t || r < q)) { const int d = s_first[v] + r; if (d < keep) lb[d] = la[i]; }
    }
    if (tid == 0) B.cnt_b[sg] = keep;
}
// e. the Harris response (orb.cu:93-138) of the kept candidates of every segment, one a lane
__global__ void __launch_bounds__(64) k_ob_harris(const ObTable *__restrict__ T, ObBufs B)
{
    int blk;
    const int sg = ob_find(T->harris, blockIdx.x, blk), p = blk * 64 + threadIdx.x;
    const ObSeg &s = T->segs[sg];
    if (p >= min(B.cnt_b[sg], s.cap_b)) return;
    const short2 l = B.loc_b[s.b_off + p];
    B.resp_b[s.b_off + p] = harris_at(s.img, s.step, l.x, l.y, 7, 0.04f);       // orb.cpp:774
}
// f. cull to n by Harris response (orb.cpp:778), the same rule with float keys: an element's output row is its rank, the number of elements that are greater, or
// equal and earlier (std::stable_sort under a > b).  A workgroup ranks 256 elements of a segment, one a lane; every key of the segment passes through LDS in tiles.
__global__ void __launch_bounds__(256) k_ob_cull_harris(const ObTable *__restrict__ T, ObBufs B)
{
    __shared__ float s_key[OB_SORT_TILE];
    int blk;
    const int sg = ob_find(T->sort, blockIdx.x, blk), tid = threadIdx.x, idx = blk * 256 + tid;
    const ObSeg &s = T->segs[sg];
    const int c = min(B.cnt_b[sg], s.cap_b), keep = s.cap_c;
    const short2 *lb = B.loc_b + s.b_off;
    const float *rb = B.resp_b + s.b_off;
    short2 *lc = B.loc_c + s.c_off;
    float *rc = B.resp_c + s.c_off;
    if (idx == 0) B.cnt_c[sg] = min(c, keep);
    if (c <= keep) {
        if (idx < c) { lc[idx] = lb[idx]; rc[idx] = rb[idx]; }
        return;
    }
    if (blk * 256 >= c) return;                                 // (the whole workgroup)
    const float key = idx < c ? rb[idx] : 0.f;
    int rank = 0;
    for (int t0 = 0; t0 < c; t0 += OB_SORT_TILE) {
        const int m = min(OB_SORT_TILE, c - t0);
        __syncthreads();                                        // the tile before is read
        for (int j = tid; j < m; j += 256) s_key[j] = rb[t0 + j];
        __syncthreads();
        for (int j = 0; j < m; ++j) {
            const float kj = s_key[j];                          // one address a workgroup: a broadcast
            rank += (kj > key) || (kj == key && t0 + j < idx);
        }
    }
    if (idx < c && rank < keep) { lc[rank] = lb[idx]; rc[rank] = key; }
}
// g. a keypoint's row in its view: the counts of the view's lower levels, then its place in its own
__device__ __forceinline__ int ob_view_row(const ObTable *__restrict__ T, const int *__restrict__ cnt_c, int sg, int p)
{
    int row = p;
    for (int k = T->segs[sg].first; k < sg; ++k) row += cnt_c[k];
    return row;
}
// the intensity-centroid angle (orb.cpp:780; orb.cu:160-211) and mergeKeyPoints' six floats (:823-865): x, y, response, angle, octave, size
__global__ void __launch_bounds__(64) k_ob_finish(const ObTable *__restrict__ T, ObBufs B)
{
    int blk;
    const int sg = ob_find(T->finish, blockIdx.x, blk), p = blk * 64 + threadIdx.x;
    const ObSeg &s = T->segs[sg];
    if (p >= min(B.cnt_c[sg], s.cap_c)) return;
    const int row = ob_view_row(T, B.cnt_c, sg, p);
    if (row >= B.max_keypoints) return;                         // the host fails the call; nothing is written past the view's rows
    const short2 l = B.loc_c[s.c_off + p];
    float *k = B.kp + 6 * ((size_t)s.view * B.max_keypoints + row);
    k[0] = (float)l.x * s.loc_scale; k[1] = (float)l.y * s.loc_scale; k[2] = B.resp_c[s.c_off + p];
    k[3] = ic_angle_at(s.img, s.step, l.x, l.y, B.half, T->umax);
    k[4] = (float)s.level; k[5] = s.size;
}
// the descriptors (orb.cpp:783-821): byte b of keypoint p a lane, 8 keypoints a workgroup, straight into the view's descriptor matrix
__global__ void __launch_bounds__(256) k_ob_desc(const ObTable *__restrict__ T, ObBufs B)
{
    int blk;
    const int sg = ob_find(T->desc, blockIdx.x, blk), b = threadIdx.x & 31, p = blk * 8 + (threadIdx.x >> 5);
    const ObSeg &s = T->segs[sg];
    if (p >= min(B.cnt_c[sg], s.cap_c)) return;
    const int row = ob_view_row(T, B.cnt_c, sg, p);
    if (row >= B.max_keypoints) return;
    const short2 l = B.loc_c[s.c_off + p];
    const float angle = B.kp[6 * ((size_t)s.view * B.max_keypoints + row) + 3];
    s.desc[(size_t)row * s.dstep + b] = (uint8_t)orb_desc_byte(s.img, s.step, l.x, l.y, angle, b);
}

static inline size_t ob_align(size_t n) { return (n + 255) & ~(size_t)255; }
template <int N> static inline void ob_add(ObList<N> &L, int seg, long long items)
{
    if (items <= 0) return;
    L.seg[L.n] = seg; L.start[L.n] = L.total; L.total += (int)items; L.start[++L.n] = L.total;
}

// The parameter and per-view checks of both ORB entry points (the arrays are not null); MS_ERR_INVALID names the call and, where a view is at fault, the view.
int orb_check(const char *fn, int n_views, const ms_image *gray, const ms_image *masks, const ms_orb_params *prm, int max_keypoints, const ms_image *desc)
{
    MS_CHECK(prm->nlevels >= 1 && prm->nlevels <= 16 && prm->first_level == 0 && prm->patch_size == 31 && prm->nfeatures >= 1 && prm->scale_factor > 1.f,
             "%s: supports first_level 0, patch_size 31 (the learned pattern), 1..16 levels", fn);
    // the device kernels read a (rotated) 31-px patch, the 15-px intensity-centroid disc and the 7 x 7 Harris block + Sobel halo around every keypoint WITHOUT bounds
    // checks: keypoints must keep the creator's border (orb.cpp:686-689, edgeThreshold 31 by default; 19 = ceil(18.4) is the reach of the rotated pattern);
    // a FAST threshold of 0 would make score 0 -- "no corner" in the score map -- a valid corner (fast.cu:224-282 has the same encoding), 255 can never fire
    MS_CHECK(prm->edge_threshold >= 19 && prm->edge_threshold >= prm->patch_size / 2 + 1 && prm->fast_threshold >= 1 && prm->fast_threshold <= 254,
             "%s: edge_threshold %d must be >= 19 and fast_threshold %d in [1, 254]", fn, prm->edge_threshold, prm->fast_threshold);
    MS_CHECK(max_keypoints >= prm->nfeatures, "%s: max_keypoints %d must be >= nfeatures %d", fn, max_keypoints, prm->nfeatures);
    for (int v = 0; v < n_views; ++v) {
        MS_CHECK(gray[v].data && gray[v].type == MS_8UC1, "%s: view %d: gray must be a device 8UC1 image", fn, v);
        MS_CHECK(gray[v].rows >= 0 && gray[v].cols >= 0 && gray[v].rows <= 32767 && gray[v].cols <= 32767, "%s: view %d: %d x %d is no image size", fn, v, gray[v].cols, gray[v].rows);      // (short2 coordinates)
        MS_CHECK(!masks || !masks[v].data || (masks[v].type == MS_8UC1 && masks[v].rows == gray[v].rows && masks[v].cols == gray[v].cols),
                 "%s: view %d: mask must be 8UC1 of the image size", fn, v);
        MS_CHECK(desc[v].data && desc[v].type == MS_8UC1 && desc[v].cols == 32 && desc[v].rows >= max_keypoints && desc[v].step >= 32,
                 "%s: view %d: descriptors must be 8UC1 max_keypoints x 32", fn, v);
    }
    for (int v = 0; v < n_views; ++v)                                       // the byte ranges of the descriptor matrices, steps included
        for (int u = 0; u < v; ++u) {
            const char *a0 = (const char *)desc[u].data, *a1 = a0 + (size_t)(max_keypoints - 1) * desc[u].step + 32;
            const char *b0 = (const char *)desc[v].data, *b1 = b0 + (size_t)(max_keypoints - 1) * desc[v].step + 32;
            MS_CHECK(a1 <= b0 || b1 <= a0, "%s: view %d: its descriptors overlap those of view %d", fn, v, u);
        }
    return MS_OK;
}

// the arguments are checked (orb_check) and a device is present
int orb_batch(const char *fn, int n_views, const ms_image *gray, const ms_image *masks, const ms_orb_params *prm, float *kp_host, int max_keypoints, ms_image *desc,
              int *n_out, ms_stream stream)
{
    hipStream_t st = as_stream(stream);
    const int half = prm->patch_size / 2;
    // the table: built in pinned memory with arena offsets in place of pointers, which are added once the arena is there
    const size_t o_tab = 0, o_cnt_ab = ob_align(sizeof(ObTable)), o_cnt = o_cnt_ab + ob_align(2 * sizeof(int) * OB_MAX_SEG), o_kp = o_cnt + ob_align(sizeof(int) * OB_MAX_SEG),
                 kp_bytes = sizeof(float) * 6 * (size_t)n_views * max_keypoints, back_bytes = ob_align(sizeof(int) * OB_MAX_SEG) + kp_bytes;
    char *pin = (char *)pinned_scratch().get(o_kp + kp_bytes);
    if (!pin) return fail(MS_ERR_NOMEM, "%s: cannot allocate pinned staging memory", fn);
    ObTable &T = *new (pin + o_tab) ObTable();
    {   // u_max of the circular patch (orb.cpp:514-529)
        std::vector<int> u(half + 2, 0);
        const float r2 = std::sqrt(2.f);
        for (int v = 0; v <= half * r2 / 2 + 1; ++v) u[v] = (int)std::nearbyint(std::sqrt((float)(half * half - v * v)));
        for (int v = half, v0 = 0; v >= half * r2 / 2; --v) { while (u[v0] == u[v0 + 1]) ++v0; u[v] = v0; ++v0; }
        for (size_t i = 0; i < u.size() && i < 32; ++i) T.umax[i] = u[i];
    }
    // per-level budgets (orb.cpp:501-512)
    std::vector<int> nper(prm->nlevels);
    {
        const float factor = 1.0f / prm->scale_factor;
        float nd = (float)((double)(prm->nfeatures * (1.0f - factor)) / (1.0 - std::pow((double)factor, prm->nlevels)));
        int sum = 0;
        for (int l = 0; l < prm->nlevels - 1; ++l) { nper[l] = (int)std::nearbyint(nd); sum += nper[l]; nd *= factor; }
        nper[prm->nlevels - 1] = prm->nfeatures - sum;        // may be 0 or negative (the rounding of the other levels): such a level is skipped below
    }
    auto level_scale = [&](int l) { return (float)std::pow((double)prm->scale_factor, l - prm->first_level); };     // getScale: pow(float, int) -> double -> float
    int n_seg = 0;
    long long rows = 0, na = 0, nb = 0, nc = 0;
    size_t arena = 0;                                          // pyramid levels >= 1, their masks, the score maps
    std::vector<size_t> o_img(OB_MAX_SEG, 0), o_msk(OB_MAX_SEG, 0), o_score(OB_MAX_SEG, 0);
    for (int v = 0; v < n_views; ++v) {
        const bool have_mask = masks && masks[v].data;
        const int first = n_seg;
        for (int level = 0; level < prm->nlevels; ++level) {
            const float sc = 1.0f / level_scale(level);
            const int w = (int)std::nearbyint((float)gray[v].cols * sc), h = (int)std::nearbyint((float)gray[v].rows * sc);      // cvRound(image.cols * scale)  orb.cpp:668
            if (w < 8 || h < 8) break;
            const int sg = n_seg++;
            ObSeg &s = T.segs[sg];
            s.w = w; s.h = h; s.view = v; s.level = level; s.first = first;
            s.desc = (uint8_t *)desc[v].data; s.dstep = desc[v].step;
            if (level == 0) {
                s.img = (const uint8_t *)gray[v].data; s.step = gray[v].step;
                if (have_mask) { s.mask = (const uint8_t *)masks[v].data; s.mstep = masks[v].step; }
            } else {
                const ObSeg &below = T.segs[sg - 1];
                s.ifx = (float)(1.0 / ((double)w / below.w)); s.ify = (float)(1.0 / ((double)h / below.h));      // launch_resize_linear with fx = fy = 0
                o_img[sg] = arena; arena += ob_align((size_t)w * h); s.step = (size_t)w;
                if (have_mask) { o_msk[sg] = arena; arena += ob_align((size_t)w * h); s.mstep = (size_t)w; }
                ob_add(T.pyr[level], sg, (long long)div_up(w, 64) * div_up(h, 4));
            }
            const float sf = level_scale(level);
            s.loc_scale = level != prm->first_level ? sf : 1.0f; s.size = (float)prm->patch_size * sf;
            s.n = nper[level];
            s.max_npoints = (int)(0.05 * ((double)w * h));                  // fastDetector_->setMaxNumPoints(0.05 * area)  orb.cpp:753
            // A budget <= 0 (nfeatures 7 at the defaults gives the last level -1; the reference is undefined there: its cull() releases the buffer and keeps
            // the count): the level contributes no keypoints, and nothing but its pyramid image, which the next level is resized from, is computed.
            if (s.n <= 0) continue;
            s.cap_b = (int)std::min<long long>(s.max_npoints, 2ll * s.n); s.cap_c = std::min(s.max_npoints, s.n);
            o_score[sg] = arena; arena += ob_align((size_t)w * h);
            s.row_off = (int)rows; s.a_off = (int)na; s.b_off = (int)nb; s.c_off = (int)nc;
            rows += h; na += s.max_npoints; nb += s.cap_b; nc += s.cap_c;
            ob_add(T.active, sg, 1);
            ob_add(T.tiles, sg, (long long)div_up(w, 64) * div_up(h, 4));
            ob_add(T.rows, sg, h);
            ob_add(T.harris, sg, div_up(s.cap_b, 64));
            ob_add(T.sort, sg, div_up(s.cap_b, 256));
            ob_add(T.finish, sg, div_up(s.cap_c, 64));
            ob_add(T.desc, sg, div_up(s.cap_c, 8));
            if (na > INT_MAX / 16 || T.tiles.total > INT_MAX / 16) return fail(MS_ERR_INVALID, "%s: view %d: the views are more than one batch holds", fn, v);
        }
    }
    const size_t o_rowraw = o_kp + ob_align(kp_bytes), o_rowcnt = o_rowraw + ob_align(sizeof(int) * (size_t)rows),
                 o_loc_a = o_rowcnt + ob_align(sizeof(int) * (size_t)rows), o_score_a = o_loc_a + ob_align(sizeof(short2) * (size_t)na), o_loc_b = o_score_a + ob_align((size_t)na),
                 o_resp_b = o_loc_b + ob_align(sizeof(short2) * (size_t)nb), o_loc_c = o_resp_b + ob_align(sizeof(float) * (size_t)nb),
                 o_resp_c = o_loc_c + ob_align(sizeof(short2) * (size_t)nc), o_arena = o_resp_c + ob_align(sizeof(float) * (size_t)nc), dev_bytes = o_arena + arena;
    char *dev = (char *)device_scratch().get(dev_bytes);
    if (!dev) return fail(MS_ERR_NOMEM, "%s: cannot allocate %zu bytes of device scratch", fn, dev_bytes);
    for (int sg = 0; sg < n_seg; ++sg) {
        ObSeg &s = T.segs[sg];
        if (s.level > 0) { s.img = (const uint8_t *)(dev + o_arena + o_img[sg]); if (s.mstep) s.mask = (const uint8_t *)(dev + o_arena + o_msk[sg]); }
        if (s.n > 0) s.score = (uint8_t *)(dev + o_arena + o_score[sg]);
    }
    ObBufs B{};
    B.rowraw = (int *)(dev + o_rowraw); B.rowcnt = (int *)(dev + o_rowcnt);
    B.cnt_a = (int *)(dev + o_cnt_ab); B.cnt_b = B.cnt_a + OB_MAX_SEG; B.cnt_c = (int *)(dev + o_cnt);
    B.loc_a = (short2 *)(dev + o_loc_a); B.score_a = (uint8_t *)(dev + o_score_a);
    B.loc_b = (short2 *)(dev + o_loc_b); B.resp_b = (float *)(dev + o_resp_b);
    B.loc_c = (short2 *)(dev + o_loc_c); B.resp_c = (float *)(dev + o_resp_c);
    B.kp = (float *)(dev + o_kp); B.max_keypoints = max_keypoints; B.half = half;
    const ObTable *dT = (const ObTable *)(dev + o_tab);
    const int n_active = T.active.n;

    // the pass: 1 upload, 1 clear (the block is reused: every count of this call starts at 0), nlevels + 10 launches at most, 1 copy back, 1 synchronise
    auto enqueue = [&]() -> hipError_t {
        hipError_t e = hipMemcpyAsync(dev + o_tab, pin + o_tab, sizeof(ObTable), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemsetAsync(dev + o_cnt_ab, 0, o_kp - o_cnt_ab, st);      // the three count arrays lie together
        for (int level = 1; level < prm->nlevels && e == hipSuccess; ++level) {
            if (!T.pyr[level].total) break;
            k_ob_pyramid<<<T.pyr[level].total, dim3(64, 4), 0, st>>>(dT, level);
            e = hipGetLastError();
        }
        if (!n_active || e != hipSuccess) return e;             // (never a launch with an empty grid)
        k_ob_fast<<<T.tiles.total, dim3(64, 4), 0, st>>>(dT, prm->edge_threshold, prm->fast_threshold);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        const int row_blocks = div_up(T.rows.total, 4);
        k_ob_rows<0><<<row_blocks, 256, 0, st>>>(dT, B);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        k_ob_scan<<<n_active, 256, 0, st>>>(dT, B.rowraw, nullptr);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        k_ob_rows<1><<<row_blocks, 256, 0, st>>>(dT, B);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        k_ob_scan<<<n_active, 256, 0, st>>>(dT, B.rowcnt, B.cnt_a);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        k_ob_rows<2><<<row_blocks, 256, 0, st>>>(dT, B);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        k_ob_cull_fast<<<n_active, 64 * OB_CULL_WAVES, 0, st>>>(dT, B);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        k_ob_harris<<<T.harris.total, 64, 0, st>>>(dT, B);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        k_ob_cull_harris<<<T.sort.total, 256, 0, st>>>(dT, B);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        k_ob_finish<<<T.finish.total, 64, 0, st>>>(dT, B);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        k_ob_desc<<<T.desc.total, 256, 0, st>>>(dT, B);
        return hipGetLastError();
    };
    hipError_t e = enqueue();
    if (e == hipSuccess) e = hipMemcpyAsync(pin + o_cnt, dev + o_cnt, back_bytes, hipMemcpyDeviceToHost, st);
    const hipError_t se = hipStreamSynchronize(st);            // also after a failed enqueue: nothing of this call stays in flight over the scratch blocks
    MS_HIP(e);
    MS_HIP(se);
    const int *cnt_c = (const int *)(pin + o_cnt);
    std::vector<int> total(n_views, 0);
    for (int sg = 0; sg < n_seg; ++sg) {
        const ObSeg &s = T.segs[sg];
        if (s.n <= 0) continue;
        if (cnt_c[sg] < 0 || cnt_c[sg] > s.cap_c) return fail(MS_ERR_HIP, "%s: view %d: the device returned an impossible keypoint count (%d of %d)", fn, s.view, cnt_c[sg], s.cap_c);
        total[s.view] += cnt_c[sg];
    }
    for (int v = 0; v < n_views; ++v)
        if (total[v] > max_keypoints) return fail(MS_ERR_INVALID, "%s: view %d: more than max_keypoints (%d) keypoints", fn, v, max_keypoints);
    for (int v = 0; v < n_views; ++v) {
        memcpy(kp_host + 6 * (size_t)max_keypoints * v, pin + o_kp + sizeof(float) * 6 * (size_t)max_keypoints * v, sizeof(float) * 6 * (size_t)total[v]);
        n_out[v] = total[v];
    }
    return MS_OK;
}

}  // namespace
}  // namespace ms

using namespace ms;

extern "C" {

int ms_orb_default_params(ms_orb_params *p)
{
    if (!p) return fail(MS_ERR_INVALID, "ms_orb_default_params: null");
    p->nfeatures = 2500; p->scale_factor = 1.2f; p->nlevels = 8;          // cuda::ORB::create(2500, 1.2f, 8), featurefinder.cpp:15
    p->edge_threshold = 31; p->first_level = 0; p->patch_size = 31; p->fast_threshold = 20;      // cuda::ORB::create defaults (cudafeatures2d.hpp)
    return MS_OK;
}

int ms_orb_detect_and_compute(const ms_image *gray, const ms_image *mask, const ms_orb_params *prm, float *kp_host, int max_keypoints,
                              ms_image *desc, int *n_out, ms_stream stream)
{
    const char *fn = "ms_orb_detect_and_compute";
    if (int e = require_device()) return e;
    MS_CHECK(gray && prm && kp_host && desc && n_out, "%s: bad argument", fn);
    MS_CHECK(!mask || mask->data, "%s: mask must be 8UC1 of the image size", fn);      // (in a batch a mask without data means "none"; here NULL does)
    if (int e = orb_check(fn, 1, gray, mask, prm, max_keypoints, desc)) return e;
    return orb_batch(fn, 1, gray, mask, prm, kp_host, max_keypoints, desc, n_out, stream);      // the batch of one
}

int ms_orb_detect_and_compute_batch(int n_views, const ms_image *gray, const ms_image *masks, const ms_orb_params *prm, float *kp_host, int max_keypoints,
                                    ms_image *desc, int *n_out, ms_stream stream)
{
    const char *fn = "ms_orb_detect_and_compute_batch";
    MS_CHECK(n_views >= 1 && n_views <= MS_MAX_VIEWS, "%s: n_views = %d must be in [1, %d]", fn, n_views, MS_MAX_VIEWS);
    MS_CHECK(gray, "%s: null gray", fn);
    MS_CHECK(prm, "%s: null prm", fn);
    MS_CHECK(kp_host, "%s: null keypoints_host", fn);
    MS_CHECK(desc, "%s: null descriptors", fn);
    MS_CHECK(n_out, "%s: null n_keypoints", fn);
    if (int e = orb_check(fn, n_views, gray, masks, prm, max_keypoints, desc)) return e;
    if (int e = require_device()) return e;
    return orb_batch(fn, n_views, gray, masks, prm, kp_host, max_keypoints, desc, n_out, stream);
}

int ms_feature_mask(const ms_image *img, int a_x0, int a_w, int b_x0, int b_w, ms_image *mask, ms_stream stream)
{
    if (int e = require_device()) return e;
    MS_CHECK(img && mask && img->data && mask->data && img->type == MS_8UC3 && mask->type == MS_8UC1 && img->rows == mask->rows && img->cols == mask->cols,
             "ms_feature_mask: need an 8UC3 image and an 8UC1 mask of the same size");
    k_feature_mask<<<dim3(div_up(img->cols, 64), div_up(img->rows, 4)), dim3(64, 4), 0, as_stream(stream)>>>(
        (const uint8_t *)img->data, img->step, img->rows, img->cols, a_x0, a_x0 + a_w, b_x0, b_x0 + b_w, (uint8_t *)mask->data, mask->step);
    MS_LAUNCH_CHECK();
    return MS_OK;
}

int ms_feature_inputs_batch(int n_views, const ms_image *views, const int *bands, ms_image *gray, ms_image *masks, ms_stream stream)
{
    const char *fn = "ms_feature_inputs_batch";
    MS_CHECK(n_views >= 1 && n_views <= MS_MAX_VIEWS, "%s: n_views = %d must be in [1, %d]", fn, n_views, MS_MAX_VIEWS);
    MS_CHECK(views, "%s: null warped_views", fn);
    MS_CHECK(gray || masks, "%s: gray and masks are both null: nothing to write", fn);
    MS_CHECK(!masks || bands, "%s: masks need bands", fn);
    FiTable T{};
    T.n = n_views;
    long long blocks = 0;
    for (int v = 0; v < n_views; ++v) {
        const ms_image &im = views[v];
        MS_CHECK(im.data, "%s: view %d: null warped view", fn, v);
        MS_CHECK(im.rows > 0 && im.cols > 0, "%s: view %d: empty warped view %dx%d", fn, v, im.cols, im.rows);
        MS_CHECK(im.type == MS_8UC3, "%s: view %d: warped view of type %d (need 8UC3)", fn, v, im.type);
        MS_CHECK(im.step >= (size_t)im.cols * 3, "%s: view %d: warped view step %zu smaller than a row (%zu bytes)", fn, v, im.step, (size_t)im.cols * 3);
        FiView &V = T.v[v];
        V.src = (const uint8_t *)im.data; V.sstep = im.step; V.w = im.cols; V.h = im.rows;
        const ms_image *outs[2] = {gray ? gray + v : nullptr, masks ? masks + v : nullptr};
        for (int k = 0; k < 2; ++k) {
            const ms_image *o = outs[k];
            const char *what = k ? "mask" : "gray";
            if (!o) continue;
            MS_CHECK(o->data, "%s: view %d: null %s image", fn, v, what);
            MS_CHECK(o->type == MS_8UC1, "%s: view %d: %s image of type %d (need 8UC1)", fn, v, what, o->type);
            MS_CHECK(o->rows == im.rows && o->cols == im.cols, "%s: view %d: %s image %dx%d, its view %dx%d: size mismatch", fn, v, what, o->cols, o->rows, im.cols, im.rows);
            MS_CHECK(o->step >= (size_t)o->cols, "%s: view %d: %s image step %zu smaller than a row (%d bytes)", fn, v, what, o->step, o->cols);
            (k ? V.mask : V.gray) = (uint8_t *)o->data;
            (k ? V.mstep : V.gstep) = o->step;
        }
        if (masks) {                                    // x0 + width as ms_feature_mask forms it, held inside the int range
            const int *b = bands + 4 * v;
            auto end = [](int x0, int w) { const long long e = (long long)x0 + w; return (int)std::min<long long>(std::max<long long>(e, INT_MIN), INT_MAX); };
            V.ax0 = b[0]; V.ax1 = end(b[0], b[1]); V.bx0 = b[2]; V.bx1 = end(b[2], b[3]);
        }
        V.tiles_x = div_up(im.cols, 256);
        V.block0 = (int)blocks;
        blocks += (long long)V.tiles_x * div_up(im.rows, 4);
        MS_CHECK(blocks <= INT_MAX, "%s: view %d: the views up to this one hold more than 2^31 - 1 tiles of 256 x 4 pixels", fn, v);
    }
    if (int e = require_device()) return e;
    k_feature_inputs<<<(unsigned)blocks, dim3(64, 4), 0, as_stream(stream)>>>(T);
    MS_LAUNCH_CHECK();
    return MS_OK;
}

int ms_find_homography_ransac(const float *src_xy, const float *dst_xy, int n, double reproj_threshold, int max_iters, double confidence,
                              double *H_out, uint8_t *inlier_mask, int *n_inliers, ms_stream stream)
{
    if (int e = require_device()) return e;
    MS_CHECK(src_xy && dst_xy && H_out && n >= 0, "ms_find_homography_ransac: bad argument");
    const int offsets[2] = {0, n};                                         // the batch of one
    int status = 1;
    if (int e = ransac_batch("ms_find_homography_ransac", 1, offsets, src_xy, dst_xy, reproj_threshold, max_iters, confidence, H_out, inlier_mask, n_inliers, &status, stream))
        return e;
    return status;                                                         // 1: no model (the reference returns an empty Mat)
}

int ms_find_homography_ransac_batch(int n_problems, const int *offsets, const float *src_xy, const float *dst_xy, double reproj_threshold, int max_iters, double confidence,
                                    double *H_out, uint8_t *inlier_mask, int *n_inliers, int *status, ms_stream stream)
{
    const char *fn = "ms_find_homography_ransac_batch";
    MS_CHECK(n_problems >= 0, "%s: n_problems = %d must not be negative", fn, n_problems);
    if (n_problems == 0) return MS_OK;
    MS_CHECK(offsets, "%s: null offsets", fn);
    MS_CHECK(H_out, "%s: null H", fn);
    MS_CHECK(status, "%s: null status", fn);
    MS_CHECK(offsets[0] == 0, "%s: offsets[0] = %d must be 0", fn, offsets[0]);
    for (int p = 0; p < n_problems; ++p)
        MS_CHECK(offsets[p + 1] >= offsets[p], "%s: offsets descend at problem %d (%d after %d)", fn, p, offsets[p + 1], offsets[p]);
    MS_CHECK(offsets[n_problems] == 0 || src_xy, "%s: null src_xy with %d points", fn, offsets[n_problems]);
    MS_CHECK(offsets[n_problems] == 0 || dst_xy, "%s: null dst_xy with %d points", fn, offsets[n_problems]);
    MS_CHECK(std::isfinite(reproj_threshold), "%s: reproj_threshold is not finite", fn);
    MS_CHECK(std::isfinite(confidence), "%s: confidence is not finite", fn);
    if (int e = require_device()) return e;
    return ransac_batch(fn, n_problems, offsets, src_xy, dst_xy, reproj_threshold, max_iters, confidence, H_out, inlier_mask, n_inliers, status, stream);
}

}  // extern "C"
