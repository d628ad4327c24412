// pair_match.hip -- every view pair of a rig matched in one call (gfx950): detail::BestOf2NearestMatcher / BestOf2NearestRangeMatcher
// (OCV/stitching/src/matchers.cpp:248-297 two-direction 2-NN + ratio test + cross-check, :692-770 homography and confidence, :784-808 candidate pairs),
// then the two host steps that follow it in Stitcher::estimateCameraParams: leaveBiggestComponent (motion_estimators.cpp:1041-1097) and waveCorrect (:892-970).
//
// Two launches whatever the number of pairs.  k_pair_knn2: the grid is laid over a table of (directed pair, first query) entries; a workgroup scores 64
// queries (one a lane, the descriptor in registers) against tiles of 256 train rows staged in LDS -- a train row comes from L2 once per workgroup and tile,
// every LDS read is a broadcast --, its four waves take a quarter of the tile each and merge their (distance, index)-ordered best pairs at the end.
// k_pair_select: one workgroup a pair applies the ratio test and the cross-check and compacts with a ballot / prefix scan, so the list order is exact and
// no atomic assigns a position.  Integer work but for the one float compare of the ratio test (-ffp-contract=off: one multiply, one compare).
// ms_match_lists is the application's own rule (360_stitcher/featurefinder.cpp:48-170: one direction, the 0.7 ratio test in double, no cross-check) over an explicit
// list of directed problems: the same k_pair_knn2 over the same tables, then k_list_select, one workgroup a problem.
#include <cfloat>
#include <climits>
#include <cmath>
#include <vector>
#include "common.hpp"

namespace ms {
namespace {

constexpr int PM_QUERIES = 64;         // queries a workgroup: one a lane
constexpr int PM_TILE = 256;           // train rows a tile: 8 KiB of LDS at 32 bytes a row, 16 KiB at 64
constexpr int PM_THREADS = 256;

struct PmView { const uint8_t *desc; size_t step; int n, pad; };
struct PmSeg { int qview, tview; unsigned knn_off, pad; };             // a directed pair: the rows of qview against the rows of tview (>= 2 of them)
struct PmBlock { int seg, q0; };
struct PmPair { int na, nb; unsigned knn_ab, knn_ba, slot_off, pad; };   // a pair with both views non-empty; its list has room for na + nb slots

// ms_knn_match_hamming2's order, as matcher.hip states it (that unit is left as it is: its object file stays byte-identical)
struct Best2 { int d0, j0, d1, j1; };

__device__ __forceinline__ bool before(int da, int ja, int db, int jb) { return da < db || (da == db && ja < jb); }

__device__ __forceinline__ void insert(Best2 &b, int d, int j)
{
    if (before(d, j, b.d0, b.j0)) { b.d1 = b.d0; b.j1 = b.j0; b.d0 = d; b.j0 = j; }
    else if (before(d, j, b.d1, b.j1)) { b.d1 = d; b.j1 = j; }
}

// knn[seg.knn_off + q] = (j0, d0, j1, d1): ms_knn_match_hamming2's rule.  Only directed pairs whose train side has two rows or more are in the table.
template <int WORDS>
__global__ void __launch_bounds__(PM_THREADS) k_pair_knn2(const PmView *__restrict__ views, const PmSeg *__restrict__ segs, const PmBlock *__restrict__ blocks, int words,
                                                          int4 *__restrict__ knn)
{
    constexpr int MAXW = WORDS ? WORDS : 16;
    __shared__ __attribute__((aligned(16))) unsigned tile[PM_TILE * MAXW];
    __shared__ int4 part[PM_THREADS / 64 - 1][64];
    const PmBlock blk = blocks[blockIdx.x];
    const PmSeg seg = segs[blk.seg];
    const PmView qv = views[seg.qview], tv = views[seg.tview];
    const int W = WORDS ? WORDS : words;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = blk.q0 + lane;
    const bool live = q < qv.n;
    unsigned qw[MAXW];
    const unsigned *qp = (const unsigned *)(qv.desc + (size_t)(live ? q : blk.q0) * qv.step);      // (blk.q0 < qv.n: the table holds no empty block)
#pragma unroll
    for (int k = 0; k < MAXW; ++k) qw[k] = k < W ? qp[k] : 0u;
    Best2 b{INT_MAX, INT_MAX, INT_MAX, INT_MAX};          // index INT_MAX = "none": sorts after every real row
    for (int t0 = 0; t0 < tv.n; t0 += PM_TILE) {
        const int rows = min(PM_TILE, tv.n - t0);
        __syncthreads();                                  // the previous tile has been scored by every wave
        for (int i = threadIdx.x; i < rows * W; i += PM_THREADS) {
            const int r = i / W, k = i - r * W;
            tile[i] = ((const unsigned *)(tv.desc + (size_t)(t0 + r) * tv.step))[k];
        }
        __syncthreads();
        const int r1 = min(rows, wave * 64 + 64);
#pragma unroll 4
        for (int r = wave * 64; r < r1; ++r) {
            const unsigned *tp = tile + r * W;
            int d = 0;
#pragma unroll
            for (int k = 0; k < MAXW; ++k)
                if (k < W) d += __popc(qw[k] ^ tp[k]);
            insert(b, d, t0 + r);
        }
    }
    if (wave) part[wave - 1][lane] = make_int4(b.d0, b.j0, b.d1, b.j1);
    __syncthreads();
    if (wave == 0 && live) {
        for (int w = 0; w < PM_THREADS / 64 - 1; ++w) {
            const int4 o = part[w][lane];
            insert(b, o.x, o.y);
            insert(b, o.z, o.w);
        }
        knn[seg.knn_off + q] = make_int4(b.j0, b.d0, b.j1, b.d1);
    }
}

// the position of a passing thread among the passing threads of the workgroup, in thread order; total = how many pass.  Called by every thread.
__device__ __forceinline__ int block_rank(bool pass, int *wsum, int &total)
{
    const unsigned long long m = __ballot(pass);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();                                      // the previous round's sums have been read
    if (lane == 0) wsum[wave] = __popcll(m);
    __syncthreads();
    int off = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < PM_THREADS / 64; ++w) { const int c = wsum[w]; off += w < wave ? c : 0; total += c; }
    return off + __popcll(m & ((1ull << lane) - 1ull));
}

__device__ __forceinline__ bool ratio_pass(const int4 e, float t) { return (float)e.y < t * (float)e.w; }

// slots[p.slot_off ..]: the pair's list, query | train << 16 (both below 2^15) and the distance; hdr[pair] = (count, n_forward)
__global__ void __launch_bounds__(PM_THREADS) k_pair_select(const PmPair *__restrict__ pairs, const int4 *__restrict__ knn, float t, int2 *__restrict__ hdr,
                                                            uint2 *__restrict__ slots)
{
    __shared__ int wsum[PM_THREADS / 64];
    const PmPair p = pairs[blockIdx.x];
    uint2 *out = slots + p.slot_off;
    int base = 0, total;
    if (p.nb >= 2)
        for (int q0 = 0; q0 < p.na; q0 += PM_THREADS) {
            const int q = q0 + (int)threadIdx.x;
            int4 e = make_int4(0, 0, 0, 0);
            bool pass = false;
            if (q < p.na) { e = knn[p.knn_ab + q]; pass = ratio_pass(e, t); }
            const int pos = block_rank(pass, wsum, total);
            if (pass) out[base + pos] = make_uint2((unsigned)q | ((unsigned)e.x << 16), (unsigned)e.y);
            base += total;
        }
    const int n_forward = base;
    if (p.na >= 2)
        for (int q0 = 0; q0 < p.nb; q0 += PM_THREADS) {
            const int q = q0 + (int)threadIdx.x;
            int4 e = make_int4(0, 0, 0, 0);
            bool pass = false;
            if (q < p.nb) { e = knn[p.knn_ba + q]; pass = ratio_pass(e, t); }
            if (pass && p.nb >= 2) {                      // (j0, q) already listed: row j0 of a passed and its nearest row is q
                const int4 f = knn[p.knn_ab + e.x];
                if (f.x == q && ratio_pass(f, t)) pass = false;
            }
            const int pos = block_rank(pass, wsum, total);
            if (pass) out[base + pos] = make_uint2((unsigned)e.x | ((unsigned)q << 16), (unsigned)e.y);
            base += total;
        }
    if (threadIdx.x == 0) hdr[blockIdx.x] = make_int2(base, n_forward);
}

// A problem of ms_match_lists with a query row and two train rows or more: its 2-NN rows at knn_off, room for nq slots at slot_off
struct PmList { int nq; unsigned knn_off, slot_off, pad; };

// featurefinder::matchFeatures' rule (featurefinder.cpp:62-66) over one directed problem a workgroup: row q passes iff (double)d0 < ratio * (double)d1 -- one double
// multiply, one compare --, the passing rows compacted in query order through block_rank, slots as k_pair_select writes them; hdr[problem] = count
__global__ void __launch_bounds__(PM_THREADS) k_list_select(const PmList *__restrict__ lists, const int4 *__restrict__ knn, double ratio, int *__restrict__ hdr,
                                                            uint2 *__restrict__ slots)
{
    __shared__ int wsum[PM_THREADS / 64];
    const PmList p = lists[blockIdx.x];
    uint2 *out = slots + p.slot_off;
    int base = 0, total;
    for (int q0 = 0; q0 < p.nq; q0 += PM_THREADS) {
        const int q = q0 + (int)threadIdx.x;
        int4 e = make_int4(0, 0, 0, 0);
        bool pass = false;
        if (q < p.nq) { e = knn[p.knn_off + q]; pass = (double)e.y < ratio * (double)e.w; }
        const int pos = block_rank(pass, wsum, total);
        if (pass) out[base + pos] = make_uint2((unsigned)q | ((unsigned)e.x << 16), (unsigned)e.y);
        base += total;
    }
    if (threadIdx.x == 0) hdr[blockIdx.x] = base;
}

size_t pm_align(size_t n) { return (n + 255) & ~(size_t)255; }

// the rules ms_match_pairs and ms_match_lists share for their feature tables (`what`: "view" / "set") and RANSAC parameters; *bytes: the descriptor length, 0 where no entry has rows
int pm_check_features(const char *fn, const char *what, int n, const ms_view_features *views, int *bytes_out)
{
    int bytes = 0;
    for (int v = 0; v < n; ++v) {
        const ms_view_features &f = views[v];
        MS_CHECK(f.n_keypoints >= 0 && f.n_keypoints <= MS_MATCH_MAX_KEYPOINTS, "%s: %s %d: n_keypoints %d outside [0, %d]", fn, what, v, f.n_keypoints, MS_MATCH_MAX_KEYPOINTS);
        MS_CHECK(f.n_keypoints <= f.descriptors.rows, "%s: %s %d: n_keypoints %d above descriptors.rows %d", fn, what, v, f.n_keypoints, f.descriptors.rows);
        MS_CHECK(f.keypoint_stride >= 2, "%s: %s %d: keypoint_stride %d below 2", fn, what, v, f.keypoint_stride);
        MS_CHECK(f.width >= 1 && f.height >= 1, "%s: %s %d: image size (width, height) %d x %d", fn, what, v, f.width, f.height);
        if (f.n_keypoints == 0) continue;
        MS_CHECK(f.keypoints, "%s: %s %d: null keypoints", fn, what, v);
        MS_CHECK(f.descriptors.data, "%s: %s %d: null descriptors", fn, what, v);
        MS_CHECK(f.descriptors.type == MS_8UC1, "%s: %s %d: descriptors type %d (need 8UC1)", fn, what, v, f.descriptors.type);
        MS_CHECK(f.descriptors.cols > 0 && f.descriptors.cols % 4 == 0 && f.descriptors.cols <= 64, "%s: %s %d: descriptor length %d (need a multiple of 4 up to 64 bytes)", fn, what,
                 v, f.descriptors.cols);
        MS_CHECK(f.descriptors.step % 4 == 0 && f.descriptors.step >= (size_t)f.descriptors.cols && (uintptr_t)f.descriptors.data % 4 == 0,
                 "%s: %s %d: descriptors step %zu / data must be 4-byte aligned and the step not below the row", fn, what, v, f.descriptors.step);
        MS_CHECK(bytes == 0 || bytes == f.descriptors.cols, "%s: %s %d: descriptor length %d differs from %d of an earlier %s", fn, what, v, f.descriptors.cols, bytes, what);
        bytes = f.descriptors.cols;
    }
    *bytes_out = bytes;
    return MS_OK;
}

int pm_check_ransac(const char *fn, double reproj_threshold, int max_iters, double confidence)
{
    MS_CHECK(std::isfinite(reproj_threshold) && reproj_threshold >= 0.0 && max_iters >= 0 && std::isfinite(confidence) && confidence >= 0.0 && confidence < 1.0,
             "%s: ransac_reproj_threshold / ransac_max_iters / ransac_confidence = %g / %d / %g (0 = the default; confidence below 1)", fn, reproj_threshold, max_iters, confidence);
    return MS_OK;
}

// k_pair_knn2's tables for one more directed segment, the rows of view q against the rows of view t (two of them or more): returns the segment's offset into knn
unsigned pm_add_segment(const std::vector<PmView> &hv, int q, int t, std::vector<PmSeg> &segs, std::vector<PmBlock> &blocks, size_t &knn_n)
{
    const unsigned off = (unsigned)knn_n;
    for (int q0 = 0; q0 < hv[q].n; q0 += PM_QUERIES) blocks.push_back(PmBlock{(int)segs.size(), q0});
    segs.push_back(PmSeg{q, t, off, 0u});
    knn_n += (size_t)hv[q].n;
    return off;
}

std::vector<PmView> pm_views(int n, const ms_view_features *views)
{
    std::vector<PmView> hv(n);
    for (int v = 0; v < n; ++v) hv[v] = PmView{(const uint8_t *)views[v].descriptors.data, views[v].descriptors.step, views[v].n_keypoints, 0};
    return hv;
}

// the 2-NN launch over those tables (descriptors of `bytes` bytes; 32 is the specialised kernel)
hipError_t pm_launch_knn2(const PmView *dv, const PmSeg *ds, const PmBlock *db, unsigned n_blocks, int bytes, int4 *knn, hipStream_t st)
{
    if (bytes == 32) k_pair_knn2<8><<<n_blocks, PM_THREADS, 0, st>>>(dv, ds, db, 8, knn);
    else k_pair_knn2<0><<<n_blocks, PM_THREADS, 0, st>>>(dv, ds, db, bytes / 4, knn);
    return hipGetLastError();
}

double pm_det3(const double *H)
{
    return H[0] * (H[4] * H[8] - H[5] * H[7]) - H[1] * (H[3] * H[8] - H[5] * H[6]) + H[2] * (H[3] * H[7] - H[4] * H[6]);
}

// cyclic Jacobi on a symmetric 3 x 3: A -> eigenvalues on the diagonal, V's columns the eigenvectors
void pm_jacobi3(double A[3][3], double V[3][3])
{
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 64; ++sweep) {
        const double off = std::fabs(A[0][1]) + std::fabs(A[0][2]) + std::fabs(A[1][2]);
        if (off == 0.0) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                if (A[p][q] == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 3; ++k) { const double akp = A[k][p], akq = A[k][q]; A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq; }
                for (int k = 0; k < 3; ++k) { const double apk = A[p][k], aqk = A[q][k]; A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk; }
                A[p][q] = A[q][p] = 0.0;                  // (what the rotation makes of it, up to rounding)
                for (int k = 0; k < 3; ++k) { const double vkp = V[k][p], vkq = V[k][q]; V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq; }
            }
    }
}

void pm_cross(const double a[3], const double b[3], double o[3])
{
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}

}  // namespace
}  // namespace ms

using namespace ms;

extern "C" {

int ms_pair_match_default_params(ms_pair_match_params *prm)
{
    MS_CHECK(prm, "ms_pair_match_default_params: null params");
    *prm = ms_pair_match_params{};
    prm->struct_size = (unsigned)sizeof(ms_pair_match_params);
    prm->match_conf = 0.3f; prm->num_matches_thresh1 = 6; prm->num_matches_thresh2 = 6; prm->range_width = 0; prm->pair_mask = nullptr;
    prm->ransac_reproj_threshold = 0.0; prm->ransac_max_iters = 0; prm->ransac_confidence = 0.0;
    return MS_OK;
}

int ms_match_pairs(int n_views, const ms_view_features *views, const ms_pair_match_params *prm, ms_pair_matches *pairs_out, int pairs_cap, int *n_pairs,
                   ms_feature_match *matches_out, int matches_cap, int *n_matches, ms_stream stream)
{
    const char *fn = "ms_match_pairs";
    MS_CHECK(views && prm && pairs_out && n_pairs && matches_out && n_matches, "%s: null argument", fn);
    MS_CHECK(n_views >= 2 && n_views <= MS_MAX_VIEWS, "%s: n_views = %d outside [2, %d]", fn, n_views, MS_MAX_VIEWS);
    MS_CHECK(prm->struct_size == sizeof(ms_pair_match_params), "%s: params struct_size %u, this library's is %zu", fn, prm->struct_size, sizeof(ms_pair_match_params));
    MS_CHECK(std::isfinite(prm->match_conf) && prm->match_conf >= 0.f && prm->match_conf < 1.f, "%s: match_conf %g outside [0, 1)", fn, (double)prm->match_conf);
    MS_CHECK(prm->num_matches_thresh1 >= 0 && prm->num_matches_thresh2 >= 0, "%s: num_matches_thresh1 / num_matches_thresh2 = %d / %d must not be negative", fn,
             prm->num_matches_thresh1, prm->num_matches_thresh2);
    MS_CHECK(prm->range_width >= 0, "%s: range_width %d must not be negative", fn, prm->range_width);
    if (int e = pm_check_ransac(fn, prm->ransac_reproj_threshold, prm->ransac_max_iters, prm->ransac_confidence)) return e;
    MS_CHECK(pairs_cap >= 0 && matches_cap >= 0, "%s: pairs_cap / matches_cap = %d / %d must not be negative", fn, pairs_cap, matches_cap);
    int bytes = 0;
    if (int e = pm_check_features(fn, "view", n_views, views, &bytes)) return e;
    // the candidate pairs (matchers.cpp:794-798)
    std::vector<int> cand;
    for (int i = 0; i < n_views - 1; ++i)
        for (int j = i + 1; j < n_views; ++j) {
            if (prm->range_width > 0 && j >= i + prm->range_width) continue;
            if (prm->pair_mask && !prm->pair_mask[i * n_views + j]) continue;
            cand.push_back(i * n_views + j);
        }
    const int np = (int)cand.size();
    MS_CHECK(pairs_cap >= np, "%s: pairs_cap %d below the %d candidate pairs", fn, pairs_cap, np);
    if (int e = require_device()) return e;
    hipStream_t st = as_stream(stream);

    // tables: views, directed pairs, (directed pair, first query) blocks, active pairs
    const std::vector<PmView> hv = pm_views(n_views, views);
    std::vector<PmSeg> segs;
    std::vector<PmBlock> blocks;
    std::vector<PmPair> active;
    std::vector<int> active_of(np, -1);
    size_t knn_n = 0, slot_n = 0;
    for (int k = 0; k < np; ++k) {
        const int a = cand[k] / n_views, b = cand[k] % n_views, na = hv[a].n, nb = hv[b].n;
        if (na == 0 || nb == 0) continue;
        PmPair p{na, nb, 0u, 0u, (unsigned)slot_n, 0u};
        for (int dir = 0; dir < 2; ++dir) {
            const int qv = dir ? b : a, tv = dir ? a : b;
            if (hv[tv].n < 2) continue;
            (dir ? p.knn_ba : p.knn_ab) = pm_add_segment(hv, qv, tv, segs, blocks, knn_n);
        }
        active_of[k] = (int)active.size();
        active.push_back(p);
        slot_n += (size_t)(na + nb);
    }
    const int n_active = (int)active.size();
    std::vector<int2> hdr(n_active);
    std::vector<uint2> slots;
    if (n_active) {
        const size_t o_views = 0, o_segs = o_views + pm_align(hv.size() * sizeof(PmView)), o_blocks = o_segs + pm_align(segs.size() * sizeof(PmSeg)),
                     o_pairs = o_blocks + pm_align(blocks.size() * sizeof(PmBlock)), up_bytes = o_pairs + pm_align(active.size() * sizeof(PmPair));
        const size_t o_knn = up_bytes, o_out = o_knn + pm_align(knn_n * sizeof(int4)), o_slots = pm_align((size_t)n_active * sizeof(int2)),
                     out_bytes = o_slots + slot_n * sizeof(uint2);
        char *dev = (char *)device_scratch().get(o_out + out_bytes);         // per-thread grow-only block: see DeviceScratch (common.hpp)
        if (!dev) return fail(MS_ERR_NOMEM, "%s: cannot allocate %zu bytes of device scratch", fn, o_out + out_bytes);
        char *pin = (char *)pinned_scratch().get(up_bytes + out_bytes);
        if (!pin) return fail(MS_ERR_NOMEM, "%s: cannot allocate pinned staging memory", fn);
        memcpy(pin + o_views, hv.data(), hv.size() * sizeof(PmView));
        if (!segs.empty()) memcpy(pin + o_segs, segs.data(), segs.size() * sizeof(PmSeg));
        if (!blocks.empty()) memcpy(pin + o_blocks, blocks.data(), blocks.size() * sizeof(PmBlock));
        memcpy(pin + o_pairs, active.data(), active.size() * sizeof(PmPair));
        hipError_t e = hipMemcpyAsync(dev, pin, up_bytes, hipMemcpyHostToDevice, st);
        if (e == hipSuccess && !blocks.empty())
            e = pm_launch_knn2((const PmView *)(dev + o_views), (const PmSeg *)(dev + o_segs), (const PmBlock *)(dev + o_blocks), (unsigned)blocks.size(), bytes,
                               (int4 *)(dev + o_knn), st);
        if (e == hipSuccess) {
            k_pair_select<<<n_active, PM_THREADS, 0, st>>>((const PmPair *)(dev + o_pairs), (const int4 *)(dev + o_knn), 1.f - prm->match_conf, (int2 *)(dev + o_out),
                                                           (uint2 *)(dev + o_out + o_slots));
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(pin + up_bytes, dev + o_out, out_bytes, hipMemcpyDeviceToHost, st);
        const hipError_t se = hipStreamSynchronize(st);      // also after a failed enqueue: nothing of this call stays in flight over the scratch blocks
        MS_HIP(e);
        MS_HIP(se);
        memcpy(hdr.data(), pin + up_bytes, (size_t)n_active * sizeof(int2));
        slots.resize(slot_n);
        if (slot_n) memcpy(slots.data(), pin + up_bytes + o_slots, slot_n * sizeof(uint2));      // (ms_find_homography_ransac below stages through the same pinned block)
    }
    long long total = 0;
    for (int k = 0; k < n_active; ++k) {
        if (hdr[k].x < 0 || hdr[k].x > active[k].na + active[k].nb || hdr[k].y < 0 || hdr[k].y > hdr[k].x)
            return fail(MS_ERR_HIP, "%s: the device returned an impossible match count (%d, %d) for an active pair", fn, hdr[k].x, hdr[k].y);
        total += hdr[k].x;
    }
    *n_pairs = np;
    *n_matches = (int)total;
    MS_CHECK(total <= matches_cap, "%s: matches_cap %d below the %lld matches found (*n_matches holds the number)", fn, matches_cap, total);

    int first = 0;
    // BestOf2NearestMatcher::match (matchers.cpp:699-770) over all pairs in two batched rounds; per pair the rule is the reference's, line for line
    std::vector<int> round1, off1(1, 0);                  // round 1: every pair with count >= num_matches_thresh1, its centred points at off1
    std::vector<float> src, dst;
    for (int k = 0; k < np; ++k) {
        ms_pair_matches &pm = pairs_out[k];
        pm = ms_pair_matches{};
        const int a = cand[k] / n_views, b = cand[k] % n_views;
        pm.view_a = a; pm.view_b = b; pm.first = first;
        if (active_of[k] < 0) continue;
        const int count = hdr[active_of[k]].x;
        pm.count = count; pm.n_forward = hdr[active_of[k]].y;
        const uint2 *sl = slots.data() + active[active_of[k]].slot_off;
        ms_feature_match *m = matches_out + first;
        for (int i = 0; i < count; ++i) m[i] = ms_feature_match{(int)(sl[i].x & 0xffffu), (int)(sl[i].x >> 16), (int)sl[i].y, 0};
        first += count;
        if (count < prm->num_matches_thresh1) continue;
        const ms_view_features &fa = views[a], &fb = views[b];
        const size_t o = src.size();
        src.resize(o + 2 * (size_t)count); dst.resize(o + 2 * (size_t)count);
        for (int i = 0; i < count; ++i) {
            const float *pa = fa.keypoints + (size_t)m[i].query * fa.keypoint_stride, *pb = fb.keypoints + (size_t)m[i].train * fb.keypoint_stride;
            src[o + 2 * i] = pa[0] - fa.width * 0.5f; src[o + 2 * i + 1] = pa[1] - fa.height * 0.5f;
            dst[o + 2 * i] = pb[0] - fb.width * 0.5f; dst[o + 2 * i + 1] = pb[1] - fb.height * 0.5f;
        }
        round1.push_back(k);
        off1.push_back(off1.back() + count);
    }
    if (round1.empty()) return MS_OK;
    const int n1 = (int)round1.size();
    std::vector<double> Hs(9 * (size_t)n1);
    std::vector<uint8_t> mask((size_t)off1.back() + 1, 0);
    std::vector<int> st1(n1, 1);
    if (int rc = ms_find_homography_ransac_batch(n1, off1.data(), src.data(), dst.data(), prm->ransac_reproj_threshold, prm->ransac_max_iters, prm->ransac_confidence, Hs.data(),
                                                 mask.data(), nullptr, st1.data(), stream))
        return rc;
    std::vector<int> round2, off2(1, 0);                  // round 2: the inliers alone of every pair whose model passed the determinant test with num_inliers >= thresh2
    std::vector<float> src_in, dst_in;
    for (int r = 0; r < n1; ++r) {
        ms_pair_matches &pm = pairs_out[round1[r]];
        if (st1[r] != 0) continue;                        // no model: have_H = 0
        memcpy(pm.H, &Hs[9 * (size_t)r], sizeof(pm.H));
        pm.have_H = 1;
        if (std::fabs(pm_det3(pm.H)) < DBL_EPSILON) continue;
        ms_feature_match *m = matches_out + pm.first;
        const uint8_t *mk = mask.data() + off1[r];
        const float *s = src.data() + 2 * (size_t)off1[r], *d = dst.data() + 2 * (size_t)off1[r];
        pm.num_inliers = 0;
        for (int i = 0; i < pm.count; ++i) { m[i].inlier = mk[i] ? 1 : 0; pm.num_inliers += m[i].inlier; }
        pm.confidence = pm.num_inliers / (8 + 0.3 * pm.count);
        if (pm.confidence > 3.) pm.confidence = 0.;
        if (pm.num_inliers < prm->num_matches_thresh2) continue;
        for (int i = 0; i < pm.count; ++i)
            if (m[i].inlier) { src_in.push_back(s[2 * i]); src_in.push_back(s[2 * i + 1]); dst_in.push_back(d[2 * i]); dst_in.push_back(d[2 * i + 1]); }
        round2.push_back(round1[r]);
        off2.push_back(off2.back() + pm.num_inliers);
    }
    if (round2.empty()) return MS_OK;
    const int n2 = (int)round2.size();
    std::vector<int> st2(n2, 1);
    Hs.assign(9 * (size_t)n2, 0.0);
    if (int rc = ms_find_homography_ransac_batch(n2, off2.data(), src_in.data(), dst_in.data(), prm->ransac_reproj_threshold, prm->ransac_max_iters, prm->ransac_confidence,
                                                 Hs.data(), nullptr, nullptr, st2.data(), stream))
        return rc;
    for (int r = 0; r < n2; ++r) {
        ms_pair_matches &pm = pairs_out[round2[r]];
        memcpy(pm.H, &Hs[9 * (size_t)r], sizeof(pm.H));   // (no model: zeros, as the single call leaves them)
        if (st2[r] != 0) pm.have_H = 0;
    }
    return MS_OK;
}

int ms_list_match_default_params(ms_list_match_params *prm)
{
    MS_CHECK(prm, "ms_list_match_default_params: null params");
    *prm = ms_list_match_params{};
    prm->struct_size = (unsigned)sizeof(ms_list_match_params);
    prm->ratio = 0.7; prm->find_homography = 1;
    prm->ransac_reproj_threshold = 0.0; prm->ransac_max_iters = 0; prm->ransac_confidence = 0.0;
    return MS_OK;
}

int ms_match_lists(int n_sets, const ms_view_features *sets, int n_problems, const ms_match_problem *problems, const ms_list_match_params *prm, ms_pair_matches *out,
                   ms_feature_match *matches_out, int matches_cap, int *n_matches, ms_stream stream)
{
    const char *fn = "ms_match_lists";
    MS_CHECK(sets && problems && prm && out && matches_out && n_matches, "%s: null argument", fn);
    MS_CHECK(n_sets >= 1 && n_sets <= 2 * MS_MAX_VIEWS, "%s: n_sets = %d outside [1, %d]", fn, n_sets, 2 * MS_MAX_VIEWS);
    MS_CHECK(n_problems >= 0 && n_problems <= MS_MATCH_MAX_PROBLEMS, "%s: n_problems = %d outside [0, %d]", fn, n_problems, MS_MATCH_MAX_PROBLEMS);
    MS_CHECK(prm->struct_size == sizeof(ms_list_match_params), "%s: params struct_size %u, this library's is %zu", fn, prm->struct_size, sizeof(ms_list_match_params));
    MS_CHECK(std::isfinite(prm->ratio) && prm->ratio > 0.0 && prm->ratio <= 1.0, "%s: ratio %g outside (0, 1]", fn, prm->ratio);
    if (int e = pm_check_ransac(fn, prm->ransac_reproj_threshold, prm->ransac_max_iters, prm->ransac_confidence)) return e;
    MS_CHECK(matches_cap >= 0, "%s: matches_cap = %d must not be negative", fn, matches_cap);
    for (int p = 0; p < n_problems; ++p)
        MS_CHECK(problems[p].query_set >= 0 && problems[p].query_set < n_sets && problems[p].train_set >= 0 && problems[p].train_set < n_sets,
                 "%s: problem %d names the sets (query_set, train_set) %d, %d outside [0, %d)", fn, p, problems[p].query_set, problems[p].train_set, n_sets);
    int bytes = 0;
    if (int e = pm_check_features(fn, "set", n_sets, sets, &bytes)) return e;
    *n_matches = 0;
    if (n_problems == 0) return MS_OK;
    if (int e = require_device()) return e;
    hipStream_t st = as_stream(stream);

    // tables: sets, one directed segment and one list for every problem with a query row and two train rows or more, (segment, first query) blocks
    const std::vector<PmView> hv = pm_views(n_sets, sets);
    std::vector<PmSeg> segs;
    std::vector<PmBlock> blocks;
    std::vector<PmList> active;
    std::vector<int> active_of(n_problems, -1);
    size_t knn_n = 0;
    for (int p = 0; p < n_problems; ++p) {
        const int q = problems[p].query_set, t = problems[p].train_set;
        if (hv[q].n < 1 || hv[t].n < 2) continue;
        active_of[p] = (int)active.size();
        const unsigned slot_off = (unsigned)knn_n;        // a list has room for one slot a query row: slots and 2-NN rows share their offsets
        active.push_back(PmList{hv[q].n, pm_add_segment(hv, q, t, segs, blocks, knn_n), slot_off, 0u});
    }
    const int n_active = (int)active.size();
    const size_t slot_n = knn_n;
    std::vector<int> hdr(n_active);
    std::vector<uint2> slots;
    if (n_active) {
        const size_t o_views = 0, o_segs = o_views + pm_align(hv.size() * sizeof(PmView)), o_blocks = o_segs + pm_align(segs.size() * sizeof(PmSeg)),
                     o_lists = o_blocks + pm_align(blocks.size() * sizeof(PmBlock)), up_bytes = o_lists + pm_align(active.size() * sizeof(PmList));
        const size_t o_knn = up_bytes, o_out = o_knn + pm_align(knn_n * sizeof(int4)), o_slots = pm_align((size_t)n_active * sizeof(int)),
                     out_bytes = o_slots + slot_n * sizeof(uint2);
        char *dev = (char *)device_scratch().get(o_out + out_bytes);         // per-thread grow-only block: see DeviceScratch (common.hpp)
        if (!dev) return fail(MS_ERR_NOMEM, "%s: cannot allocate %zu bytes of device scratch", fn, o_out + out_bytes);
        char *pin = (char *)pinned_scratch().get(up_bytes + out_bytes);
        if (!pin) return fail(MS_ERR_NOMEM, "%s: cannot allocate pinned staging memory", fn);
        memcpy(pin + o_views, hv.data(), hv.size() * sizeof(PmView));
        memcpy(pin + o_segs, segs.data(), segs.size() * sizeof(PmSeg));
        memcpy(pin + o_blocks, blocks.data(), blocks.size() * sizeof(PmBlock));
        memcpy(pin + o_lists, active.data(), active.size() * sizeof(PmList));
        hipError_t e = hipMemcpyAsync(dev, pin, up_bytes, hipMemcpyHostToDevice, st);
        if (e == hipSuccess)                               // (an active problem has a query row, so a block)
            e = pm_launch_knn2((const PmView *)(dev + o_views), (const PmSeg *)(dev + o_segs), (const PmBlock *)(dev + o_blocks), (unsigned)blocks.size(), bytes,
                               (int4 *)(dev + o_knn), st);
        if (e == hipSuccess) {
            k_list_select<<<n_active, PM_THREADS, 0, st>>>((const PmList *)(dev + o_lists), (const int4 *)(dev + o_knn), prm->ratio, (int *)(dev + o_out),
                                                           (uint2 *)(dev + o_out + o_slots));
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(pin + up_bytes, dev + o_out, out_bytes, hipMemcpyDeviceToHost, st);
        const hipError_t se = hipStreamSynchronize(st);      // also after a failed enqueue: nothing of this call stays in flight over the scratch blocks
        MS_HIP(e);
        MS_HIP(se);
        memcpy(hdr.data(), pin + up_bytes, (size_t)n_active * sizeof(int));
        slots.resize(slot_n);
        memcpy(slots.data(), pin + up_bytes + o_slots, slot_n * sizeof(uint2));      // (ms_find_homography_ransac_batch below stages through the same pinned block)
    }
    long long total = 0;
    for (int k = 0; k < n_active; ++k) {
        if (hdr[k] < 0 || hdr[k] > active[k].nq) return fail(MS_ERR_HIP, "%s: the device returned an impossible match count %d for a problem of %d query rows", fn, hdr[k], active[k].nq);
        total += hdr[k];
    }
    *n_matches = (int)total;
    MS_CHECK(total <= matches_cap, "%s: matches_cap %d below the %lld matches found (*n_matches holds the number)", fn, matches_cap, total);

    // featurefinder.cpp:68-106 for every non-empty list in one batched round: centred points, findHomography(RANSAC), the inlier count; confidence 1
    std::vector<int> round, off(1, 0);
    std::vector<float> src, dst;
    int first = 0;
    for (int p = 0; p < n_problems; ++p) {
        ms_pair_matches &pm = out[p];
        pm = ms_pair_matches{};
        pm.view_a = problems[p].query_set; pm.view_b = problems[p].train_set; pm.first = first; pm.confidence = 1.0;
        if (active_of[p] < 0) continue;
        const int count = hdr[active_of[p]];
        pm.count = pm.n_forward = count;
        const uint2 *sl = slots.data() + active[active_of[p]].slot_off;
        ms_feature_match *m = matches_out + first;
        for (int i = 0; i < count; ++i) m[i] = ms_feature_match{(int)(sl[i].x & 0xffffu), (int)(sl[i].x >> 16), (int)sl[i].y, 0};
        first += count;
        if (!prm->find_homography || count < 1) continue;
        const ms_view_features &fa = sets[pm.view_a], &fb = sets[pm.view_b];
        const size_t o = src.size();
        src.resize(o + 2 * (size_t)count); dst.resize(o + 2 * (size_t)count);
        for (int i = 0; i < count; ++i) {
            const float *pa = fa.keypoints + (size_t)m[i].query * fa.keypoint_stride, *pb = fb.keypoints + (size_t)m[i].train * fb.keypoint_stride;
            src[o + 2 * i] = pa[0] - fa.width * 0.5f; src[o + 2 * i + 1] = pa[1] - fa.height * 0.5f;
            dst[o + 2 * i] = pb[0] - fb.width * 0.5f; dst[o + 2 * i + 1] = pb[1] - fb.height * 0.5f;
        }
        round.push_back(p);
        off.push_back(off.back() + count);
    }
    if (round.empty()) return MS_OK;
    const int nr = (int)round.size();
    std::vector<double> Hs(9 * (size_t)nr);
    std::vector<uint8_t> mask((size_t)off.back() + 1, 0);
    std::vector<int> status(nr, 1), inl(nr, 0);
    if (int rc = ms_find_homography_ransac_batch(nr, off.data(), src.data(), dst.data(), prm->ransac_reproj_threshold, prm->ransac_max_iters, prm->ransac_confidence, Hs.data(),
                                                 mask.data(), inl.data(), status.data(), stream))
        return rc;
    for (int r = 0; r < nr; ++r) {
        ms_pair_matches &pm = out[round[r]];
        memcpy(pm.H, &Hs[9 * (size_t)r], sizeof(pm.H));    // (no model: zeros, as the single call leaves them)
        pm.have_H = status[r] == 0;
        pm.num_inliers = inl[r];
        ms_feature_match *m = matches_out + pm.first;
        for (int i = 0; i < pm.count; ++i) m[i].inlier = mask[(size_t)off[r] + i] ? 1 : 0;
    }
    return MS_OK;
}

int ms_biggest_component(int n_views, const ms_pair_matches *pairs, int n_pairs, double conf_threshold, int *keep, int *n_keep)
{
    const char *fn = "ms_biggest_component";
    MS_CHECK(keep && n_keep && (pairs || n_pairs == 0), "%s: null argument", fn);
    MS_CHECK(n_views >= 1 && n_views <= MS_MAX_VIEWS, "%s: n_views = %d outside [1, %d]", fn, n_views, MS_MAX_VIEWS);
    MS_CHECK(n_pairs >= 0, "%s: n_pairs = %d must not be negative", fn, n_pairs);
    MS_CHECK(!std::isnan(conf_threshold), "%s: conf_threshold is not a number", fn);
    int comp[MS_MAX_VIEWS], size[MS_MAX_VIEWS] = {0};
    for (int v = 0; v < n_views; ++v) comp[v] = v;        // a component is named by its lowest view
    for (int k = 0; k < n_pairs; ++k) {
        const int a = pairs[k].view_a, b = pairs[k].view_b;
        MS_CHECK(a >= 0 && a < n_views && b >= 0 && b < n_views, "%s: pair %d names views %d, %d outside [0, %d)", fn, k, a, b, n_views);
        MS_CHECK(a != b, "%s: pair %d pairs view %d with itself", fn, k, a);
        if (!(pairs[k].confidence >= conf_threshold)) continue;
        const int lo = comp[a] < comp[b] ? comp[a] : comp[b], hi = comp[a] < comp[b] ? comp[b] : comp[a];
        for (int v = 0; v < n_views; ++v) if (comp[v] == hi) comp[v] = lo;
    }
    for (int v = 0; v < n_views; ++v) ++size[comp[v]];
    int best = 0;
    for (int v = 1; v < n_views; ++v) if (size[v] > size[best]) best = v;      // ties: the component with the lowest view
    int n = 0;
    for (int v = 0; v < n_views; ++v) if (comp[v] == best) keep[n++] = v;
    *n_keep = n;
    return MS_OK;
}

int ms_wave_correct(int n_views, const double *R_in, int kind, double *R_out)
{
    const char *fn = "ms_wave_correct";
    MS_CHECK(R_in && R_out, "%s: null argument", fn);
    MS_CHECK(n_views >= 1 && n_views <= MS_MAX_VIEWS, "%s: n_views = %d outside [1, %d]", fn, n_views, MS_MAX_VIEWS);
    MS_CHECK(kind == MS_WAVE_HORIZ || kind == MS_WAVE_VERT, "%s: kind %d (MS_WAVE_HORIZ = 0, MS_WAVE_VERT = 1)", fn, kind);
    for (int k = 0; k < 9 * n_views; ++k) MS_CHECK(std::isfinite(R_in[k]), "%s: view %d: rotation entry %d is not finite", fn, k / 9, k % 9);
    double Rc[MS_MAX_VIEWS * 9];
    memcpy(Rc, R_in, sizeof(double) * 9 * (size_t)n_views);                     // R_out may be R_in
    memcpy(R_out, Rc, sizeof(double) * 9 * (size_t)n_views);
    if (n_views <= 1) return 1;
    double A[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, V[3][3], img_k[3] = {0, 0, 0};
    for (int v = 0; v < n_views; ++v) {
        const double *R = Rc + 9 * v, x[3] = {R[0], R[3], R[6]};
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) A[i][j] += x[i] * x[j];
        img_k[0] += R[2]; img_k[1] += R[5]; img_k[2] += R[8];
    }
    pm_jacobi3(A, V);
    int order[3] = {0, 1, 2};                             // descending eigenvalues, the earlier first among equals
    for (int i = 0; i < 2; ++i) for (int j = 0; j < 2 - i; ++j) if (A[order[j]][order[j]] < A[order[j + 1]][order[j + 1]]) { const int t = order[j]; order[j] = order[j + 1]; order[j + 1] = t; }
    const int col = kind == MS_WAVE_HORIZ ? order[2] : order[0];
    double rg1[3] = {V[0][col], V[1][col], V[2][col]}, rg0[3], rg2[3];
    pm_cross(rg1, img_k, rg0);
    const double norm = std::sqrt(rg0[0] * rg0[0] + rg0[1] * rg0[1] + rg0[2] * rg0[2]);
    if (norm <= DBL_MIN) return 1;
    for (int i = 0; i < 3; ++i) rg0[i] /= norm;
    pm_cross(rg0, rg1, rg2);
    double conf = 0.0;
    for (int v = 0; v < n_views; ++v) {
        const double *R = Rc + 9 * v;
        if (kind == MS_WAVE_HORIZ) conf += rg0[0] * R[0] + rg0[1] * R[3] + rg0[2] * R[6];
        else conf -= rg1[0] * R[0] + rg1[1] * R[3] + rg1[2] * R[6];
    }
    if (conf < 0) for (int i = 0; i < 3; ++i) { rg0[i] = -rg0[i]; rg1[i] = -rg1[i]; }
    const double *G[3] = {rg0, rg1, rg2};
    for (int v = 0; v < n_views; ++v)
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c)
                R_out[9 * v + 3 * r + c] = G[r][0] * Rc[9 * v + c] + G[r][1] * Rc[9 * v + 3 + c] + G[r][2] * Rc[9 * v + 6 + c];
    return MS_OK;
}

}  // extern "C"
