// stitch_app.cpp -- C++ host pipeline over the C-ABI, with the thread / queue graph of the reference's main loop
// (360_stitcher/timed.cpp): capture -> LockableVector of the newest frame per camera -> stitch_one (upload, compositor,
// push) -> BlockingQueue -> consume (8U panorama, optional I420 for the encoder) and a recalibration thread that swaps
// CPW meshes while frames keep flowing.  No OpenCV: device images are plain HIP allocations wrapped as ms_image.
//
//   reference                                   here
//   ------------------------------------------  ---------------------------------------------------------------
//   stitch_calib / warpImages (calibration.cpp)  calibrate(): ms_set_camera/gain, ms_build_maps, ms_build_masks, ms_init_blender
//   LockableVector<Mat> imgs (lockablevector.h)  Lockable<std::vector<HostFrame>>
//   capture threads (networking.cpp / debug)     capture(): synthetic frames (same pattern as video-stitcher_amd/synth.py, noise off);
//                                                with --nv12 the cameras deliver NV12 (defs.h:10-17) and cvtColor(YUV2BGR_NV12)
//                                                (networking.cpp:45-47, CPU in the reference) runs on the device after a half-size upload
//   stitch_one (timed.cpp:123-152)               stitch_one(): hipMemcpy2DAsync x N + msshim::Compositor::stitch_one + results.push
//   BlockingQueue<GpuMat> results                BlockingQueue<Slot*>
//   consume (timed.cpp:232-330)                  consume(): optional ms_bgr_to_i420, download, checksum / dump
//   recalibrate thread (timed.cpp:414-463)       recalibrate(): ms_set_mesh per view from its own stream
//
// Usage: stitch_app [--views 6] [--size 1920x1080] [--out 3840x1920] [--hfov 90] [--bands 5] [--frames 300] [--cpw]
//                   [--i420] [--nv12 | --nv12-direct] [--dump pano.bin] [--no-upload] [--solve-mesh [--temporal ALPHA]]
//                   [--reference-calib [--work-megapix 0.6] [--seam-megapix 0.01] [--compose-megapix 1.4] [--seam-finder voronoi|dp]]
//                   [--viewport YAW,PITCH,ROLL,HFOV,WxH | --cubemap N] [--aa LEVELS | --orbit DEG]
//                   [--drop-view V:F0:F1] [--dump-frames frames.bin] [--track-gains K] [--exposure-ramp V:F] [--dump-i420 planes.bin]
//                   [--lens-brown k1,k2,p1,p2,k3 | --lens-fisheye k1,k2,k3,k4[,max_theta]]
//                   [--rig-error V:YAW:PITCH:ROLL] [--refine-rig]
// --temporal ALPHA (with --solve-mesh) switches the mesh solver's temporal term on with that weight (USE_TEMPORAL, meshwarper.cpp:121-151; ALPHAS[3], defs.h:69): from
// the second round on every view is also matched against itself one round earlier (matchFeaturesBoth: both rings in one call), the previous round's features stay
// alive for that one round, and the JSON line's "temporal_matches" sums the temporal matches handed to the solver.
// --rig-error (degrees) renders camera V's scene frames (synth_scene_frame: --solve-mesh's frames and --refine-rig's) through a rig that is really rotated by
// R_y(yaw) R_x(pitch) R_z(roll) in the camera's own frame, while calibration assumes the ideal ring.  --refine-rig runs, after the first calibration, the device
// front end between neighbouring views on the projection-warped scene frames (as --solve-mesh does every round), then ms_refine_rig with a Huber threshold of two
// warped pixels; it applies the rotations (ms_set_camera), calibrates again and prints one line "rig_refine: {...}" with the refinement's info and every view's
// angle to the rendered truth before and after, in the anchor's gauge.
// --lens-brown / --lens-fisheye give EVERY camera that lens (ms_set_lens; coefficients as OpenCV's distCoeffs / fisheye D, max_theta in degrees): maps, ROIs and,
// with --reference-calib, the seam-scale calibration come from the library's lens model, and the JSON line's "map_source" is 2 (MS_MAPS_LENS) instead of 0.
// --nv12-direct keeps BGR copies of the cameras' frames off the device in every mode: the warp samples the planes (ms_stitch_nv12), --i420 makes the encoder's
// planes in the same call (ms_stitch_nv12_i420: no 8U canvas is written; --dump, --dump-frames and --consume need the canvas and keep the two-step form
// ms_stitch_nv12 + ms_bgr_to_i420), --track-gains reads the planes (ms_track_gains_nv12).  With a compose-scale resize (--reference-calib) the frames go
// through ms_nv12_to_bgr_batch + ms_resize_linear_batch: the one-pass ms_nv12_resize_linear_batch gives the same bytes (--fused-resize selects it) but is
// measured slower than the two launches (41 against 37 us per six 1080p frames, README).  With --nv12 the exposure ramp scales the Y plane only (the camera's exposure, not its colour).
// --aa LEVELS (with --viewport or --cubemap) renders the views antialiased: the footprints are built once, beside the maps (ms_build_view_footprint), every canvas
// gets its mip chain of LEVELS levels (ms_build_pano_mips) and ms_reproject_aa samples it; the JSON line then carries "aa_levels".  Without it nothing changes.
// --orbit DEG (with --viewport or --cubemap, not with --aa) moves the virtual cameras: canvas n of the run is rendered under the rig rotation Ry(n DEG)
// (ms_look_at_view's Ry).  The pose table of the whole run is built once (ms_view_pose_table) and uploaded before the loop, laid out [frame][job][9]; the consumer
// calls ms_reproject_poses with one frame and that frame's slice.  No maps are built; the JSON line then carries "orbit_deg".
// --dump-i420 FILE writes the last frame's I420 planes (every --i420 mode); the JSON line's "i420_call" names the call that produced them.
// --track-gains K: every K-th stitch call is followed by one ms_track_gains on the stitch stream with that call's frames (exposure tracking; 0 = off, the
// default: nothing changes).  --exposure-ramp V:F multiplies camera V's synthetic frames by F from the middle of the run on, so that the tracker has a drift
// to follow without cameras.  With tracking on, the closing JSON line ends with the final gains and the solve counters.
// --drop-view: camera V delivers no new frame for the stitched frames [F0, F1).  The main loop gives every camera CAMERA_TIMEOUT_MS to deliver the frame it
// stitches next; a camera that has not is left out (ms_set_active_views), and the full set comes back when it delivers again.  The reference exits instead
// ("Failed to read all cameras", timed.cpp main loop).  --dump-frames writes every 8U panorama, in frame order, to one file.
// --reference-calib runs msshim::stitch_calib (calibration.cpp:252-311): the reference's rig and scale bookkeeping, cylindrical warper, seam-scale
// gains + Voronoi seams from the first frames, the num_bands rule, and -- with the default COMPOSE_MEGAPIX -- cuda::resize of every frame.
// Prints one JSON line: end-to-end frames/s INCLUDING the PCIe upload of every source frame (unlike bench.py).
#include <hip/hip_runtime.h>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "../shim/ms_shim.hpp"

#define HIPCHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)

// ---- the two containers of the reference's thread graph -------------------------------------------------------
template <class T> struct Lockable {           // lockablevector.h: a value + the mutex every user takes
    T v;
    std::mutex mu;
};
template <class T> class BlockingQueue {       // blockingqueue.h: unbounded push, blocking pop
public:
    void push(T x) { { std::lock_guard<std::mutex> lk(mu_); q_.push_back(std::move(x)); } cv_.notify_one(); }
    T pop() { std::unique_lock<std::mutex> lk(mu_); cv_.wait(lk, [&] { return !q_.empty(); }); T x = std::move(q_.front()); q_.pop_front(); return x; }
private:
    std::mutex mu_; std::condition_variable cv_; std::deque<T> q_;
};

// ---- a device image with the fields the shim expects (cv::cuda::GpuMat's) -------------------------------------
struct DevMat {
    int rows = 0, cols = 0, flags = 0;
    size_t step = 0;
    unsigned char *data = nullptr;
    int type() const { return flags; }
    void create(int r, int c, int t) { create(r, c, t, t == MS_8UC3 ? 3 : (t == MS_32FC1 ? 4 : (t == MS_16SC3 ? 6 : (t == MS_16SC1 ? 2 : 1)))); }    // GpuMat::create(rows, cols, type)
    void create(int r, int c, int t, int elem, bool contiguous = false)
    {
        if (data && r == rows && c == cols && t == flags) return;       // GpuMat::create is a no-op when nothing changes
        if (data) HIPCHECK(hipFree(data));
        size_t pitch = (size_t)c * elem;
        if (contiguous) HIPCHECK(hipMalloc((void **)&data, pitch * r));  // (the I420 planes are one contiguous buffer, like the Mat cvtColor fills)
        else HIPCHECK(hipMallocPitch((void **)&data, &pitch, (size_t)c * elem, r));
        rows = r; cols = c; flags = t; step = pitch;
    }
};
struct HostFrame { unsigned char *p = nullptr; int w = 0, h = 0; long long seq = -1; };   // pinned BGR frame

struct Options {
    int views = 6, w = 1920, h = 1080, out_w = 3840, out_h = 1920, bands = 5, frames = 300;
    double hfov = 90.0;
    bool cpw = false, i420 = false, upload = true, nv12 = false, solve_mesh = false;
    bool nv12_direct = false;         // --nv12-direct: no cvtColor pass at all, the warp samples the NV12 planes (ms_stitch_nv12)
    int consume_w = 0, consume_h = 0;           // > 0: consume()'s resize + black bars + BGR2YUV_I420 on the device (timed.cpp:251-316), OUTPUT_WIDTH x OUTPUT_HEIGHT
    int update_mask = 0;                        // > 0: mb->update_mask(idx, ...) after every mesh swap (timed.cpp:598-605, commented out there), enqueue-only with this margin
    bool reference_calib = false;               // stitch_calib as the reference ships it: cylindrical warper, megapixel budgets of defs.h, seam-scale pipeline
    double work_mp = 0.6, seam_mp = 0.01, compose_mp = 1.4;      // WORK_MEGAPIX, SEAM_MEAGPIX, COMPOSE_MEGAPIX (defs.h:51-53)
    std::string dump;
    int drop_view = -1, drop_f0 = 0, drop_f1 = 0;    // --drop-view V:F0:F1
    std::string dump_frames;
    int track_gains = 0;                        // --track-gains K
    int ramp_view = -1; double ramp_factor = 1.0;      // --exposure-ramp V:F
    std::string dump_i420;                      // --dump-i420 FILE
    bool viewport = false;                      // --viewport YAW,PITCH,ROLL,HFOV,WxH: a virtual pan / tilt / zoom camera rendered from the canvas (ms_reproject) in consume()
    double vp_yaw = 0, vp_pitch = 0, vp_roll = 0, vp_hfov = 90;
    int vp_w = 0, vp_h = 0;
    bool orbit = false;                         // --orbit DEG: ms_reproject_poses under the rig rotation Ry(n DEG) for canvas n, no maps
    double orbit_deg = 0.0;
    int aa = 0;                                 // --aa LEVELS: ms_build_pano_mips + ms_reproject_aa instead of ms_reproject
    int cubemap = 0;                            // --cubemap N: a 3N x 2N atlas of six N x N faces (ms_cube_face_view order, left to right, top to bottom)
    bool fused_resize = false;                  // --fused-resize: with --nv12-direct and a compose-scale resize, planes -> small_imgs in one pass
    ms_lens lens{sizeof(ms_lens), MS_LENS_NONE, {0, 0, 0, 0, 0, 0, 0, 0}, 0.0};      // --lens-brown / --lens-fisheye: every camera's lens
    int rig_err_view = -1; double rig_err_deg[3] = {0, 0, 0};    // --rig-error V:YAW:PITCH:ROLL
    bool refine_rig = false;                    // --refine-rig
    double temporal = 0.0;                      // --temporal ALPHA: the weight of the mesh solver's temporal term (0 = off, as the reference ships it)
    int seam_finder = MS_SEAM_VORONOI;          // --seam-finder voronoi | dp (with --reference-calib: what the seam-scale calibration cuts with)
};
constexpr int CAMERA_TIMEOUT_MS = 100;               // --drop-view: how long the main loop waits for a camera's frame before it stitches without it

// same pattern as synth.frame(w, h, i, t, noise=False): clip(rint(128 + 60 sin(2pi(x/97 + y/61 + i/7 + c/3)) + 40 checker))
static void synth_frame(unsigned char *dst, int w, int h, int view)
{
    const double two_pi = 2.0 * M_PI;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const double phase = x / 97.0 + y / 61.0 + view / 7.0;
            const double chk = 40.0 * (((x / 32) + (y / 32)) & 1);
            for (int c = 0; c < 3; ++c) {
                double v = 128.0 + 60.0 * std::sin(two_pi * (phase + c / 3.0)) + chk;
                v = std::nearbyint(v);
                dst[((size_t)y * w + x) * 3 + c] = (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
            }
        }
}

// A scene-consistent synthetic camera frame for --solve-mesh: a texture fixed on the viewing sphere (blocks of random grey levels: corners for FAST,
// structure for the descriptors) seen through the pinhole camera `view` of the rig, so that neighbouring warped views show the SAME content where they
// overlap and the device front-end finds real correspondences.  `shift_px` moves this camera's view of the scene by that many panorama pixels
// (a stand-in for parallax): it is what the mesh optimiser then has to absorb.
// `E` (3 x 3 row-major, may be null): the camera's real orientation inside its nominal one -- the ray of a pixel is E * (dx, dy, 1) in the ring camera's frame (--rig-error).
static void synth_scene_frame(unsigned char *dst, int w, int h, int view, int n_views, double hfov_deg, double pano_scale, double shift_px, const double *E = nullptr)
{
    const float rot = (float)(2.0 * M_PI * (double)(float)view / n_views);
    const double c = std::cos((double)rot), s = std::sin((double)rot);
    const double f = (w / 2.0) / std::tan(hfov_deg * M_PI / 180.0 / 2.0);
    const double cell = 32.0 / pano_scale;                          // blocks of 32 panorama pixels
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            double dx = (x - w / 2.0) / f, dy = (y - h / 2.0) / f, dz = 1.0;
            if (E) {
                const double ex = E[0] * dx + E[1] * dy + E[2], ey = E[3] * dx + E[4] * dy + E[5], ez = E[6] * dx + E[7] * dy + E[8];
                dx = ex; dy = ey; dz = ez;
            }
            const double X = c * dx + s * dz, Y = dy, Z = -s * dx + c * dz;           // world = R_y(rot) * camera
            const double u = std::atan2(X, Z) + shift_px / pano_scale, v = M_PI - std::acos(Y / std::sqrt(X * X + Y * Y + Z * Z));
            const long long cu = (long long)std::floor(u / cell), cv = (long long)std::floor(v / cell);
            const double fu = u / cell - cu, fv = v / cell - cv;
            for (int ch = 0; ch < 3; ++ch) {
                unsigned hsh = (unsigned)(cu * 73856093ll) ^ (unsigned)(cv * 19349663ll) ^ (unsigned)(ch * 83492791);
                hsh ^= hsh >> 13; hsh *= 0x5bd1e995u; hsh ^= hsh >> 15;
                double val = 40.0 + (double)((hsh >> 8) & 0xff) * 175.0 / 255.0;
                val += 18.0 * std::sin(2.0 * M_PI * (fu + 0.3 * ch)) * std::sin(2.0 * M_PI * fv);      // some texture inside a block
                val = std::nearbyint(val);
                dst[((size_t)y * w + x) * 3 + ch] = (unsigned char)(val < 1 ? 1 : (val > 255 ? 255 : val));    // never 0: black marks "outside the view" in createMesh's masks
            }
        }
}

// synthetic NV12 camera frame, same pattern as synth.nv12_frame: Y = the green channel of synth_frame's pattern, interleaved U/V = smooth ramps
static void synth_nv12(unsigned char *dst, int w, int h, int view)
{
    const double two_pi = 2.0 * M_PI;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const double phase = x / 97.0 + y / 61.0 + view / 7.0;
            double v = 128.0 + 60.0 * std::sin(two_pi * (phase + 1.0 / 3.0)) + 40.0 * (((x / 32) + (y / 32)) & 1);
            v = std::nearbyint(v);
            dst[(size_t)y * w + x] = (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
        }
    unsigned char *uv = dst + (size_t)w * h;
    for (int y = 0; y < h / 2; ++y)
        for (int x = 0; x < w / 2; ++x) {
            uv[(size_t)y * w + 2 * x] = (unsigned char)(64 + (3 * x + 5 * view) % 128);
            uv[(size_t)y * w + 2 * x + 1] = (unsigned char)(64 + (2 * y + 7 * view) % 128);
        }
}

// a smooth synthetic CPW mesh (the optimiser that produces real ones is out of scope): identity + amp sin(2 pi u + phase) sin(pi v)
// 3 x 3 row-major helpers of --rig-error / --refine-rig
static void mat3_mul(const double *A, const double *B, double *C)
{
    double T[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) T[r * 3 + c] = A[r * 3] * B[c] + A[r * 3 + 1] * B[3 + c] + A[r * 3 + 2] * B[6 + c];
    memcpy(C, T, sizeof(T));
}
static void mat3_t(const double *A, double *C) { double T[9]; for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) T[r * 3 + c] = A[c * 3 + r]; memcpy(C, T, sizeof(T)); }
static void rot_axis(int axis, double t, double *R)       // 0: R_x, 1: R_y (the ring's convention), 2: R_z
{
    const double c = std::cos(t), s = std::sin(t);
    const double Rx[9] = {1, 0, 0, 0, c, -s, 0, s, c}, Ry[9] = {c, 0, s, 0, 1, 0, -s, 0, c}, Rz[9] = {c, -s, 0, s, c, 0, 0, 0, 1};
    memcpy(R, axis == 0 ? Rx : (axis == 1 ? Ry : Rz), sizeof(Rx));
}
static double mat3_angle(const double *A, const double *B)      // the angle of A B^T
{
    double Bt[9], M[9];
    mat3_t(B, Bt); mat3_mul(A, Bt, M);
    const double x = M[7] - M[5], y = M[2] - M[6], z = M[3] - M[1];
    return std::atan2(0.5 * std::sqrt(x * x + y * y + z * z), 0.5 * (M[0] + M[4] + M[8] - 1.0));
}

static void make_mesh(int aw, int ah, int N, int M, double phase, double amp, std::vector<float> &mx, std::vector<float> &my)
{
    mx.resize((size_t)N * M); my.resize((size_t)N * M);
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < M; ++j) {
            const double u = (double)j / (M - 1), v = (double)i / (N - 1);
            const double d = amp * std::sin(2.0 * M_PI * u + phase) * std::sin(M_PI * v);
            mx[(size_t)i * M + j] = (float)(u * (aw - 1) + d);
            my[(size_t)i * M + j] = (float)(v * (ah - 1) + 0.5 * d);
        }
}

struct Slot {                 // one entry of the ring of caller-owned outputs (no per-frame allocation)
    DevMat pano8u, i420;
    hipEvent_t done = nullptr;
    long long seq = -1;
};

int main(int argc, char **argv)
{
    Options o;
    for (int a = 1; a < argc; ++a) {
        std::string k = argv[a];
        auto next = [&]() -> const char * { if (a + 1 >= argc) { fprintf(stderr, "missing value for %s\n", k.c_str()); exit(2); } return argv[++a]; };
        if (k == "--views") o.views = atoi(next());
        else if (k == "--size") sscanf(next(), "%dx%d", &o.w, &o.h);
        else if (k == "--out") sscanf(next(), "%dx%d", &o.out_w, &o.out_h);
        else if (k == "--hfov") o.hfov = atof(next());
        else if (k == "--bands") o.bands = atoi(next());
        else if (k == "--frames") o.frames = atoi(next());
        else if (k == "--cpw") o.cpw = true;
        else if (k == "--solve-mesh") o.cpw = o.solve_mesh = true;
        else if (k == "--update-mask") { o.cpw = true; o.update_mask = atoi(next()); }
        else if (k == "--consume") sscanf(next(), "%dx%d", &o.consume_w, &o.consume_h);
        else if (k == "--i420") o.i420 = true;
        else if (k == "--no-upload") o.upload = false;
        else if (k == "--nv12") o.nv12 = true;
        else if (k == "--nv12-direct") { o.nv12 = true; o.nv12_direct = true; }
        else if (k == "--dump") o.dump = next();
        else if (k == "--reference-calib") o.reference_calib = true;
        else if (k == "--work-megapix") o.work_mp = atof(next());
        else if (k == "--seam-megapix") o.seam_mp = atof(next());
        else if (k == "--compose-megapix") o.compose_mp = atof(next());
        else if (k == "--drop-view") {
            if (sscanf(next(), "%d:%d:%d", &o.drop_view, &o.drop_f0, &o.drop_f1) != 3 || o.drop_view < 0) { fprintf(stderr, "--drop-view wants V:F0:F1\n"); return 2; }
        }
        else if (k == "--dump-frames") o.dump_frames = next();
        else if (k == "--track-gains") o.track_gains = atoi(next());
        else if (k == "--dump-i420") o.dump_i420 = next();
        else if (k == "--viewport") {
            if (sscanf(next(), "%lf,%lf,%lf,%lf,%dx%d", &o.vp_yaw, &o.vp_pitch, &o.vp_roll, &o.vp_hfov, &o.vp_w, &o.vp_h) != 6) { fprintf(stderr, "--viewport wants YAW,PITCH,ROLL,HFOV,WxH\n"); return 2; }
            o.viewport = true;
        }
        else if (k == "--cubemap") o.cubemap = atoi(next());
        else if (k == "--aa") o.aa = atoi(next());
        else if (k == "--orbit") { o.orbit_deg = atof(next()); o.orbit = true; }
        else if (k == "--fused-resize") o.fused_resize = true;
        else if (k == "--lens-brown") {      // k1,k2,p1,p2,k3 in distCoeffs order: k3 is k[4]
            double *c = o.lens.k;
            if (sscanf(next(), "%lf,%lf,%lf,%lf,%lf", &c[0], &c[1], &c[2], &c[3], &c[4]) != 5) { fprintf(stderr, "--lens-brown wants k1,k2,p1,p2,k3\n"); return 2; }
            o.lens.model = MS_LENS_BROWN;
        } else if (k == "--lens-fisheye") {
            double *c = o.lens.k;
            if (sscanf(next(), "%lf,%lf,%lf,%lf,%lf", &c[0], &c[1], &c[2], &c[3], &o.lens.max_theta_deg) < 4) { fprintf(stderr, "--lens-fisheye wants k1,k2,k3,k4[,max_theta]\n"); return 2; }
            o.lens.model = MS_LENS_FISHEYE;
        }
        else if (k == "--refine-rig") o.refine_rig = true;
        else if (k == "--temporal") o.temporal = atof(next());
        else if (k == "--seam-finder") {
            const std::string v = next();
            if (v == "voronoi") o.seam_finder = MS_SEAM_VORONOI;
            else if (v == "dp") o.seam_finder = MS_SEAM_DP;
            else { fprintf(stderr, "--seam-finder wants voronoi or dp\n"); return 2; }
        }
        else if (k == "--rig-error") {
            if (sscanf(next(), "%d:%lf:%lf:%lf", &o.rig_err_view, &o.rig_err_deg[0], &o.rig_err_deg[1], &o.rig_err_deg[2]) != 4 || o.rig_err_view < 0) { fprintf(stderr, "--rig-error wants V:YAW:PITCH:ROLL\n"); return 2; }
        }
        else if (k == "--exposure-ramp") {
            if (sscanf(next(), "%d:%lf", &o.ramp_view, &o.ramp_factor) != 2 || o.ramp_view < 0 || o.ramp_factor < 0) { fprintf(stderr, "--exposure-ramp wants V:F\n"); return 2; }
        }
        else { fprintf(stderr, "unknown option %s\n", k.c_str()); return 2; }
    }
    if (o.drop_view >= o.views) { fprintf(stderr, "--drop-view: view %d of %d\n", o.drop_view, o.views); return 2; }
    if (o.ramp_view >= o.views) { fprintf(stderr, "--exposure-ramp: view %d of %d\n", o.ramp_view, o.views); return 2; }
    if (o.rig_err_view >= o.views) { fprintf(stderr, "--rig-error: view %d of %d\n", o.rig_err_view, o.views); return 2; }
    if (o.refine_rig && (o.reference_calib || o.nv12)) { fprintf(stderr, "stitch_app: --refine-rig is wired up for the BASELINE rig with BGR cameras (no --reference-calib, no --nv12)\n"); return 2; }
    if (o.seam_finder != MS_SEAM_VORONOI && !o.reference_calib) { fprintf(stderr, "stitch_app: --seam-finder dp needs --reference-calib (the seam-scale calibration has the images; ms_build_masks has none)\n"); return 2; }
    if (o.temporal != 0.0 && !o.solve_mesh) { fprintf(stderr, "--temporal needs --solve-mesh\n"); return 2; }
    if (!(o.temporal >= 0.0) || !std::isfinite(o.temporal)) { fprintf(stderr, "--temporal wants ALPHA >= 0\n"); return 2; }
    if (o.track_gains < 0) { fprintf(stderr, "--track-gains wants K >= 0\n"); return 2; }
    if (!o.dump_i420.empty() && !o.i420) { fprintf(stderr, "--dump-i420 needs --i420\n"); return 2; }
    if (o.viewport && o.cubemap) { fprintf(stderr, "--viewport and --cubemap exclude each other\n"); return 2; }
    if (o.cubemap < 0 || (o.cubemap && o.i420 && o.cubemap % 2)) { fprintf(stderr, "--cubemap wants N >= 1 (even with --i420)\n"); return 2; }
    if (o.aa && !(o.viewport || o.cubemap)) { fprintf(stderr, "--aa needs --viewport or --cubemap\n"); return 2; }
    if (o.orbit && !(o.viewport || o.cubemap)) { fprintf(stderr, "--orbit needs --viewport or --cubemap\n"); return 2; }
    if (o.orbit && o.aa) { fprintf(stderr, "--orbit and --aa exclude each other (ms_reproject_poses point-samples)\n"); return 2; }
    if (o.orbit && !std::isfinite(o.orbit_deg)) { fprintf(stderr, "--orbit wants a finite angle in degrees\n"); return 2; }
    if (o.aa < 0 || o.aa > MS_VIEW_MAX_LEVELS) { fprintf(stderr, "--aa wants 1..%d levels\n", (int)MS_VIEW_MAX_LEVELS); return 2; }
    if (o.viewport && o.i420 && (o.vp_w % 2 || o.vp_h % 2)) { fprintf(stderr, "--viewport with --i420 wants an even size\n"); return 2; }
    if (o.fused_resize && !o.nv12_direct) { fprintf(stderr, "--fused-resize needs --nv12-direct\n"); return 2; }
    if (ms_lens_check(&o.lens) != MS_OK) { fprintf(stderr, "stitch_app: %s\n", ms_last_error()); return 2; }
    FILE *frames_file = nullptr;       // --dump-frames (opened before any thread starts)
    if (!o.dump_frames.empty() && !(frames_file = fopen(o.dump_frames.c_str(), "wb"))) { fprintf(stderr, "cannot write %s\n", o.dump_frames.c_str()); return 2; }
    bool frames_file_ok = true;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { fprintf(stderr, "stitch_app: no HIP device (libmsstitch has no CPU fallback)\n"); return 3; }

    try {
        // ---- stitch_calib ------------------------------------------------------------------------------------
        std::unique_ptr<msshim::Compositor> comp_owner;
        msshim::Calibration cal;
        const bool with_lens = o.lens.model != MS_LENS_NONE;
        const std::vector<ms_lens> lenses((size_t)o.views, o.lens);
        if (o.reference_calib) {
            // the reference's own calibration from the first frame of every camera (device 8UC3, full size)
            std::vector<DevMat> first(o.views);
            std::vector<unsigned char> host((size_t)o.w * o.h * 3);
            for (int i = 0; i < o.views; ++i) {
                first[i].create(o.h, o.w, MS_8UC3, 3);
                synth_frame(host.data(), o.w, o.h, i);
                HIPCHECK(hipMemcpy2D(first[i].data, first[i].step, host.data(), (size_t)o.w * 3, (size_t)o.w * 3, o.h, hipMemcpyHostToDevice));
            }
            comp_owner = msshim::stitch_calib(first, MS_PROJ_CYLINDRICAL, o.cpw, cal, o.hfov, o.work_mp, o.seam_mp, o.compose_mp, 5.f, -1, -1, 1, -1, nullptr, o.cpw ? o.update_mask : 0,
                                              with_lens ? lenses.data() : nullptr, o.seam_finder);
            for (auto &m : first) HIPCHECK(hipFree(m.data));
            const ms_pano_geom g = comp_owner->panoGeom();
            o.out_w = (2 * std::max(std::abs(cal.pano_roi.x), std::abs(cal.pano_roi.x + cal.pano_roi.width)) + 1) & ~1;
            o.out_h = (2 * std::max(std::abs(cal.pano_roi.y), std::abs(cal.pano_roi.y + cal.pano_roi.height)) + 1) & ~1;
            o.bands = g.num_bands;
            fprintf(stderr, "stitch_calib: work %.4f seam %.4f compose %.4f, frames %dx%d%s, warper scale %.3f, pano %dx%d, blend width %.1f -> %d bands, gains",
                    cal.rig.work_scale, cal.rig.seam_scale, cal.rig.compose_scale, cal.rig.compose_width, cal.rig.compose_height,
                    cal.rig.resize_input ? " (resized per frame)" : "", cal.rig.compose_warp_scale, cal.pano_roi.width, cal.pano_roi.height, cal.blend_width, g.num_bands);
            for (double gn : cal.gains) fprintf(stderr, " %.3f", gn);
            fprintf(stderr, "\n");
        } else {
            // BASELINE rig: the reference's rig model at full resolution, spherical warper with the full circle on out_w columns
            cal.rig = msshim::calibrateCameras(o.views, o.w, o.h, o.hfov, -1.0, 0.01, -1.0);
            comp_owner.reset(new msshim::Compositor(o.views, o.w, o.h, MS_PROJ_SPHERICAL, (float)(o.out_w / (2.0 * M_PI)), o.bands, o.cpw, o.out_w, o.out_h, 1, o.cpw ? o.update_mask : 0));
            for (int i = 0; i < o.views; ++i) {
                comp_owner->setCamera(i, cal.rig.K_compose[i], cal.rig.R[i]);
                if (with_lens) comp_owner->setLens(i, &lenses[i]);
                comp_owner->setGain(i, 1.0 + 0.02 * (i - (o.views - 1) / 2.0));
            }
            comp_owner->buildMaps();
            comp_owner->buildMasks(true);
            comp_owner->init_gpu();
        }
        msshim::Compositor &comp = *comp_owner;
        if (o.solve_mesh && o.reference_calib && cal.rig.resize_input) { fprintf(stderr, "stitch_app: --solve-mesh with a resized compose scale is not wired up (use --compose-megapix -1)\n"); return 2; }
        const float warp_scale = o.reference_calib ? cal.rig.compose_warp_scale : (float)(o.out_w / (2.0 * M_PI));
        const bool resize_in = o.reference_calib && cal.rig.resize_input;
        const int cw = o.reference_calib ? cal.rig.compose_width : o.w, ch = o.reference_calib ? cal.rig.compose_height : o.h;
        // --nv12-direct --i420 in one call, where no 8U canvas is needed otherwise (the canvas is what --dump, --dump-frames and --consume read)
        const bool view_on = o.viewport || o.cubemap > 0;      // (the virtual cameras sample the canvas too)
        const bool nv12_i420 = o.nv12_direct && o.i420 && !resize_in && o.dump.empty() && o.dump_frames.empty() && o.consume_w <= 0 && !view_on;
        const bool fused_resize = o.fused_resize && resize_in;
        const char *i420_call = !o.i420 ? "none" : (nv12_i420 ? "ms_stitch_nv12_i420" : "ms_bgr_to_i420");
        hipStream_t stitch_stream, recal_stream;
        HIPCHECK(hipStreamCreateWithFlags(&stitch_stream, hipStreamNonBlocking));
        HIPCHECK(hipStreamCreateWithFlags(&recal_stream, hipStreamNonBlocking));
        // the scene frames' geometry: camera i really sits at R_y(shift_i / scale) R_ring_i E_i (the shift is --solve-mesh's stand-in for parallax, E --rig-error's rotation)
        std::vector<double> rig_E((size_t)9 * o.views, 0.0);
        for (int i = 0; i < o.views; ++i) {
            double *E = &rig_E[9 * (size_t)i];
            E[0] = E[4] = E[8] = 1.0;
            if (i == o.rig_err_view) {
                double Ry[9], Rx[9], Rz[9];
                rot_axis(1, o.rig_err_deg[0] * M_PI / 180.0, Ry); rot_axis(0, o.rig_err_deg[1] * M_PI / 180.0, Rx); rot_axis(2, o.rig_err_deg[2] * M_PI / 180.0, Rz);
                mat3_mul(Rx, Rz, E); mat3_mul(Ry, E, E);
            }
        }
        auto scene_shift = [&](int i) { return o.solve_mesh ? (i % 2 ? 1.0 : -1.0) * std::max(1.5, warp_scale / 200.0) : 0.0; };   // odd / even cameras see the scene +-3 px apart
        if (o.refine_rig) {
            // Stitcher::estimateCameraParams' bundle adjustment (stitching/src/stitcher.cpp:573-574) in the place the reference app leaves empty: warp the scene frames
            // with the ring's maps, createMesh's front end between neighbours (meshwarper.cpp:82-119), ms_refine_rig, and the calibration chain again
            namespace ff = msshim::featurefinder;
            std::vector<DevMat> full(o.views), images(o.views);
            std::vector<unsigned char> host((size_t)o.w * o.h * 3);
            for (int i = 0; i < o.views; ++i) {
                const ms_view_geom g = comp.viewGeom(i);
                full[i].create(o.h, o.w, MS_8UC3, 3);
                images[i].create(g.roi.height, g.roi.width, MS_8UC3, 3);
                synth_scene_frame(host.data(), o.w, o.h, i, o.views, o.hfov, warp_scale, scene_shift(i), i == o.rig_err_view ? &rig_E[9 * (size_t)i] : nullptr);
                HIPCHECK(hipMemcpy2D(full[i].data, full[i].step, host.data(), (size_t)o.w * 3, (size_t)o.w * 3, o.h, hipMemcpyHostToDevice));
                ms_image xm, ym;
                msshim::check(ms_get_maps(comp.raw(), i, &xm, &ym));
                ms_image src = msshim::wrap(full[i]), dst = msshim::wrap(images[i]);
                msshim::check(ms_remap(&src, &xm, &ym, &dst, MS_INTER_LINEAR_FIXPT, MS_BORDER_CONSTANT, (ms_stream)recal_stream));
            }
            std::vector<DevMat> fmasks;
            ff::featureMasks(images, fmasks, std::min(400, std::max(16, o.out_w / 10)), (ms_stream)recal_stream);
            std::vector<ff::ImageFeatures<DevMat>> feats;
            ff::findFeatures(images, fmasks, feats, (ms_stream)recal_stream);
            std::vector<ff::MatchesInfo> pairwise(o.views);
            ff::matchFeatures(feats, pairwise, (ms_stream)recal_stream);
            ms_rig_refine_params prm;
            msshim::check(ms_rig_refine_default_params(&prm));
            prm.huber_rad = 2.0 / warp_scale;
            std::vector<float> R_new;
            const ms_rig_refine_info info = msshim::refineRig(comp, msshim::inlierLists(feats, pairwise), R_new, &prm, (ms_stream)recal_stream);
            for (auto *v : {&full, &images, &fmasks}) for (auto &m : *v) if (m.data) HIPCHECK(hipFree(m.data));
            for (auto &f : feats) if (f.descriptors.data) HIPCHECK(hipFree(f.descriptors.data));
            // every view's angle to the rendered truth in the gauge of the held anchor: R_ring_0 R_true_0^T R_true_i
            std::vector<double> truth((size_t)9 * o.views), ring((size_t)9 * o.views);
            for (int i = 0; i < o.views; ++i) {
                double Rs[9];
                for (int k = 0; k < 9; ++k) ring[9 * (size_t)i + k] = (double)cal.rig.R[i][k];
                rot_axis(1, scene_shift(i) / warp_scale, Rs);
                mat3_mul(&ring[9 * (size_t)i], &rig_E[9 * (size_t)i], &truth[9 * (size_t)i]);
                mat3_mul(Rs, &truth[9 * (size_t)i], &truth[9 * (size_t)i]);
            }
            double G[9];
            mat3_t(&truth[0], G); mat3_mul(&ring[0], G, G);
            printf("rig_refine: {\"iterations\": %d, \"stop_reason\": %d, \"cost_initial\": %.9g, \"cost_final\": %.9g, \"matches_used\": %d, \"pairs_used\": %d, \"pairs_ignored\": %d, "
                   "\"outliers\": %d, \"max_rotation_rad\": %.9g, \"warp_scale\": %.9g", info.iterations, info.stop_reason, info.cost_initial, info.cost_final, info.matches_used,
                   info.pairs_used, info.pairs_ignored, info.outliers, info.max_rotation_rad, (double)warp_scale);
            for (int pass = 0; pass < 2; ++pass) {
                printf(", \"%s\": [", pass ? "angle_to_truth_rad" : "angle_before_rad");
                for (int i = 0; i < o.views; ++i) {
                    double want[9], got[9];
                    mat3_mul(G, &truth[9 * (size_t)i], want);
                    for (int k = 0; k < 9; ++k) got[k] = pass ? (double)R_new[9 * (size_t)i + k] : ring[9 * (size_t)i + k];
                    printf("%s%.6g", i ? ", " : "", mat3_angle(got, want));
                }
                printf("]");
            }
            printf("}\n");
            for (int i = 0; i < o.views; ++i) comp.setCamera(i, cal.rig.K_compose[i], &R_new[9 * (size_t)i]);
            comp.buildMaps();
            comp.buildMasks(true);
            comp.init_gpu();
        }
        if (o.cpw)
            for (int i = 0; i < o.views; ++i) {
                const ms_view_geom g = comp.viewGeom(i);
                std::vector<float> mx, my;
                make_mesh(g.roi.width, g.roi.height, 10, 10, 0.1 * i, 6.0, mx, my);
                comp.convertMeshToMap(i, mx.data(), my.data(), 10, 10, recal_stream);
            }

        // ---- capture side: the newest frame of every camera, in pinned memory ----------------------------------------
        Lockable<std::vector<HostFrame>> imgs;
        imgs.v.resize(o.views);
        // the cameras' frames sit back to back in ONE pinned block (view i at i * host_frame_bytes): a frame set then crosses PCIe as one copy -- six separate
        // 3 MB NV12 copies per frame cost the link 10 % in per-copy overhead (2 420 frames/s against the 2 670 the bytes allow; round 4)
        const size_t host_frame_bytes = o.nv12 ? (size_t)o.w * o.h * 3 / 2 : (size_t)o.w * o.h * 3;
        unsigned char *host_slab = nullptr;
        HIPCHECK(hipHostMalloc((void **)&host_slab, host_frame_bytes * o.views, hipHostMallocDefault));
        for (int i = 0; i < o.views; ++i) {
            HostFrame &f = imgs.v[i];
            f.w = o.w; f.h = o.h;
            f.p = host_slab + (size_t)i * host_frame_bytes;
            if (o.nv12) synth_nv12(f.p, o.w, o.h, i);          // (h * 3/2 rows of w bytes)
            else if (o.solve_mesh) synth_scene_frame(f.p, o.w, o.h, i, o.views, o.hfov, warp_scale, scene_shift(i), i == o.rig_err_view ? &rig_E[9 * (size_t)i] : nullptr);
            else synth_frame(f.p, o.w, o.h, i);
            f.seq = 0;
        }
        std::atomic<bool> running{true};
        std::atomic<long long> stitch_frame{0};          // --drop-view: the frame the main loop stitches next
        std::thread capture([&] {                       // "cameras": bump the sequence number of the frames at their own pace
            while (running.load()) {
                {
                    std::lock_guard<std::mutex> lk(imgs.mu);
                    if (o.drop_view < 0) for (auto &f : imgs.v) ++f.seq;
                    else {                              // seq = the frame a camera delivered for; camera V stalls for the frames [F0, F1)
                        const long long t = stitch_frame.load();
                        for (int i = 0; i < o.views; ++i)
                            if (!(i == o.drop_view && t >= o.drop_f0 && t < o.drop_f1)) imgs.v[i].seq = t;
                    }
                }
                std::this_thread::sleep_for(std::chrono::microseconds(200));
            }
        });

        // ---- stitch_one + results queue + consume -----------------------------------------------------------------
        // The uploaded frames are double-buffered and travel on their own stream: the H2D copies of frame t+1 overlap the stitch of frame t (the reference
        // uploads and stitches on one stream per view, timed.cpp:64-68).  up_done[b]: buffer b is filled; buf_free[b]: the stitch that read it is done.
        std::vector<DevMat> full_imgs_b[2], nv12_imgs_b[2];
        hipStream_t upload_stream;
        HIPCHECK(hipStreamCreateWithFlags(&upload_stream, hipStreamNonBlocking));
        hipEvent_t up_done[2], buf_free[2];
        bool buf_used[2] = {false, false};
        for (int b = 0; b < 2; ++b) {
            full_imgs_b[b].resize(o.views);
            if (!o.nv12) {     // BGR cameras: the same one-block layout (rows of w * 3 bytes), one copy per frame set
                unsigned char *slab = nullptr;
                HIPCHECK(hipMalloc((void **)&slab, host_frame_bytes * o.views));
                for (int i = 0; i < o.views; ++i) {
                    DevMat &m = full_imgs_b[b][i];
                    m.rows = o.h; m.cols = o.w; m.flags = MS_8UC3; m.step = (size_t)o.w * 3; m.data = slab + (size_t)i * host_frame_bytes;
                }
            } else
            for (auto &m : full_imgs_b[b]) m.create(o.h, o.w, MS_8UC3, 3);
            nv12_imgs_b[b].resize(o.nv12 ? o.views : 0);
            if (o.nv12) {      // one device block for the N NV12 frames of a set (rows of exactly `w` bytes, like the pinned block): filled by ONE copy per frame set
                unsigned char *slab = nullptr;
                HIPCHECK(hipMalloc((void **)&slab, host_frame_bytes * o.views));
                for (int i = 0; i < o.views; ++i) {
                    DevMat &m = nv12_imgs_b[b][i];
                    m.rows = o.h * 3 / 2; m.cols = o.w; m.flags = MS_8UC1; m.step = (size_t)o.w; m.data = slab + (size_t)i * host_frame_bytes;
                }
            }
            HIPCHECK(hipEventCreateWithFlags(&up_done[b], hipEventDisableTiming));
            HIPCHECK(hipEventCreateWithFlags(&buf_free[b], hipEventDisableTiming));
        }
        std::vector<DevMat> small_imgs(resize_in ? o.views : 0);
        for (auto &m : small_imgs) m.create(ch, cw, MS_8UC3, 3);
        const int RING = 4;
        std::vector<Slot> ring(RING);
        const ms_pano_geom pg = comp.panoGeom();
        int ya = pg.canvas_y & ~1, yb = std::min(o.out_h, (pg.canvas_y + pg.dst_roi_final.height + 1) & ~1);
        if (nv12_i420) { int rows = 0; comp.i420Rows(ya, rows); yb = ya + rows; }      // the span ms_stitch_nv12_i420 writes (ms_get_i420_rows)
        for (auto &s : ring) {
            s.pano8u.create(o.out_h, o.out_w, MS_8UC3, 3);
            HIPCHECK(hipMemset2D(s.pano8u.data, s.pano8u.step, 0, (size_t)o.out_w * 3, o.out_h));
            if (o.i420) {
                s.i420.create((yb - ya) * 3 / 2, o.out_w, MS_8UC1, 1, true);
                if (nv12_i420) {       // ms_stitch_nv12_i420 writes panorama pixels only: black once (Y 16, U = V 128)
                    HIPCHECK(hipMemset(s.i420.data, 16, (size_t)o.out_w * (yb - ya)));
                    HIPCHECK(hipMemset(s.i420.data + (size_t)o.out_w * (yb - ya), 128, (size_t)o.out_w * (yb - ya) / 2));
                }
            }
            HIPCHECK(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
        }
        BlockingQueue<Slot *> results, free_slots;
        for (auto &s : ring) free_slots.push(&s);

        std::vector<unsigned char> last_pano((size_t)o.out_w * o.out_h * 3);
        std::vector<unsigned char> last_i420(o.i420 ? (size_t)o.out_w * (yb - ya) * 3 / 2 : 0);
        unsigned long long checksum = 0;
        long long consumed = 0;
        DevMat encoder_frame;                           // consume(): the resized, letterboxed I420 frame the encoder gets (one buffer: the consumer is one thread)
        std::vector<unsigned char> encoder_host;
        hipStream_t consume_stream = nullptr;
        int consume_image_height = 0;
        unsigned long long consume_checksum = 0;
        if (o.consume_w > 0) {
            encoder_frame.create(o.consume_h * 3 / 2, o.consume_w, MS_8UC1, 1, true);
            encoder_host.resize((size_t)o.consume_w * o.consume_h * 3 / 2);
            HIPCHECK(hipStreamCreateWithFlags(&consume_stream, hipStreamNonBlocking));
        }
        // --viewport / --cubemap: the player's step (timed.cpp:296-300) on the device.  The maps are built once, from where the canvas lies on the sphere
        // (ms_get_pano_frame); consume() then renders every view of a frame in one ms_reproject call, as BGR or (--i420) as the encoder's planes.
        std::vector<DevMat> view_mx, view_my;
        std::vector<ms_view_job> view_jobs;
        std::vector<DevMat> view_rho;                   // --aa: the footprints, and one mips buffer (the consumer renders one canvas at a time)
        std::vector<ms_view_job_aa> view_jobs_aa;
        DevMat view_mips;
        std::vector<ms_view_pose_job> view_pose_jobs;   // --orbit: the views themselves and the run's pose table, [frame][job][9]
        DevMat view_poses;
        ms_pano_frame view_pano{};
        DevMat view_frame;
        std::vector<unsigned char> view_host;
        hipStream_t view_stream = nullptr;
        int view_w = 0, view_h = 0, view_wrap = 0, view_clamp = 0;
        unsigned long long view_checksum = 0;
        if (view_on) {
            ms_pano_frame pf;
            msshim::check(ms_get_pano_frame(comp.raw(), MS_PANO_CANVAS, &pf));
            view_wrap = pf.wrap_cols; view_clamp = pf.clamp_rows;
            view_pano = pf;
            const int n_views = o.cubemap ? 6 : 1;
            view_w = o.cubemap ? 3 * o.cubemap : o.vp_w; view_h = o.cubemap ? 2 * o.cubemap : o.vp_h;
            view_mx.resize(n_views); view_my.resize(n_views); view_jobs.resize(n_views);
            if (o.aa) { view_rho.resize(n_views); view_jobs_aa.resize(n_views); }
            HIPCHECK(hipStreamCreateWithFlags(&view_stream, hipStreamNonBlocking));
            for (int i = 0; i < n_views; ++i) {
                ms_view v;
                if (o.cubemap) msshim::check(ms_cube_face_view(i, o.cubemap, &v));
                else msshim::check(ms_look_at_view(o.vp_yaw, o.vp_pitch, o.vp_roll, o.vp_hfov, o.vp_w, o.vp_h, &v));
                if (o.orbit) { view_pose_jobs.push_back(ms_view_pose_job{v, o.cubemap ? (i % 3) * o.cubemap : 0, o.cubemap ? (i / 3) * o.cubemap : 0}); continue; }
                view_mx[i].create(v.height, v.width, MS_32FC1); view_my[i].create(v.height, v.width, MS_32FC1);
                ms_image mx = msshim::wrap(view_mx[i]), my = msshim::wrap(view_my[i]);
                msshim::check(ms_build_view_maps(&pf, &v, &mx, &my, (ms_stream)view_stream));
                view_jobs[i] = ms_view_job{mx, my, o.cubemap ? (i % 3) * o.cubemap : 0, o.cubemap ? (i / 3) * o.cubemap : 0};
                if (o.aa) {
                    view_rho[i].create(v.height, v.width, MS_32FC1);
                    ms_image rho = msshim::wrap(view_rho[i]);
                    msshim::check(ms_build_view_footprint(&pf, &mx, &my, 1.0, &rho, (ms_stream)view_stream));
                    view_jobs_aa[i] = ms_view_job_aa{view_jobs[i], rho};
                }
            }
            if (o.aa) {
                ms_mip_level lv[MS_VIEW_MAX_LEVELS];
                size_t mip_bytes = 0;
                msshim::check(ms_pano_mips_layout(o.out_w, o.out_h, o.aa, lv, &mip_bytes));
                view_mips.create(1, (int)mip_bytes, MS_8UC1, 1, true);
            }
            if (o.orbit) {
                std::vector<float> table((size_t)o.frames * n_views * 9);
                for (int n = 0; n < o.frames; ++n) {
                    const double a = n * o.orbit_deg * (M_PI / 180.0);
                    const double Ry[9] = {cos(a), 0, sin(a), 0, 1, 0, -sin(a), 0, cos(a)};
                    msshim::check(ms_view_pose_table(view_pose_jobs.data(), n_views, Ry, 1, table.data() + (size_t)n * n_views * 9));
                }
                view_poses.create(1, (int)table.size(), MS_32FC1, 4, true);
                HIPCHECK(hipMemcpy(view_poses.data, table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice));
            }
            HIPCHECK(hipStreamSynchronize(view_stream));
            if (o.i420) view_frame.create(view_h * 3 / 2, view_w, MS_8UC1, 1, true);
            else view_frame.create(view_h, view_w, MS_8UC3, 3, true);
            view_host.resize((size_t)view_w * view_h * (o.i420 ? 3 : 6) / 2);
        }
        std::thread consumer([&] {                      // consume(): wait for the frame, (I420,) bring it to the host side
            for (;;) {
                Slot *s = results.pop();
                if (!s) break;
                HIPCHECK(hipEventSynchronize(s->done));
                if (view_on) {                          // the virtual cameras' frame instead of (beside) the equirect: one launch, then the encoder's copy
                    ms_image src = msshim::wrap(s->pano8u), dst = msshim::wrap(view_frame);
                    if (o.orbit) {
                        const float *poses = (const float *)view_poses.data + (size_t)s->seq * view_pose_jobs.size() * 9;
                        msshim::check(ms_reproject_poses(&view_pano, &src, &dst, 1, view_pose_jobs.data(), (int)view_pose_jobs.size(), poses, o.i420 ? MS_VIEW_I420 : MS_VIEW_BGR,
                                                         (ms_stream)view_stream));
                    } else if (o.aa) {
                        void *mips = view_mips.data;
                        msshim::check(ms_build_pano_mips(&src, &mips, 1, o.aa, (ms_stream)view_stream));
                        msshim::check(ms_reproject_aa(&src, &mips, o.aa, &dst, 1, view_jobs_aa.data(), (int)view_jobs_aa.size(), view_wrap, view_clamp, o.i420 ? MS_VIEW_I420 : MS_VIEW_BGR,
                                                      (ms_stream)view_stream));
                    } else {
                        msshim::check(ms_reproject(&src, &dst, 1, view_jobs.data(), (int)view_jobs.size(), view_wrap, view_clamp, o.i420 ? MS_VIEW_I420 : MS_VIEW_BGR, (ms_stream)view_stream));
                    }
                    HIPCHECK(hipMemcpyAsync(view_host.data(), view_frame.data, view_host.size(), hipMemcpyDeviceToHost, view_stream));
                    HIPCHECK(hipStreamSynchronize(view_stream));
                    if (s->seq == o.frames - 1) for (unsigned char b : view_host) view_checksum = (view_checksum ^ b) * 1099511628211ull;
                }
                if (o.consume_w > 0) {                  // timed.cpp:251-316 without the download / CPU resize / CPU cvtColor: one kernel, then the encoder's copy
                    consume_image_height = msshim::consume_i420(s->pano8u, encoder_frame, o.consume_w, o.consume_h, true, (ms_stream)consume_stream);
                    HIPCHECK(hipMemcpyAsync(encoder_host.data(), encoder_frame.data, encoder_host.size(), hipMemcpyDeviceToHost, consume_stream));
                    HIPCHECK(hipStreamSynchronize(consume_stream));
                    if (s->seq == o.frames - 1) for (unsigned char b : encoder_host) consume_checksum = (consume_checksum ^ b) * 1099511628211ull;
                }
                if (nv12_i420) {                        // the encoder's input is all there is: the planes come to the host, no canvas exists
                    HIPCHECK(hipMemcpy(last_i420.data(), s->i420.data, last_i420.size(), hipMemcpyDeviceToHost));
                } else {
                if (o.i420 && !o.dump_i420.empty() && s->seq == o.frames - 1) HIPCHECK(hipMemcpy(last_i420.data(), s->i420.data, last_i420.size(), hipMemcpyDeviceToHost));
                if (s->seq == o.frames - 1 || frames_file) {           // keep the last panorama for the checksum / dump (every one for --dump-frames)
                    HIPCHECK(hipMemcpy2D(last_pano.data(), (size_t)o.out_w * 3, s->pano8u.data, s->pano8u.step, (size_t)o.out_w * 3, o.out_h, hipMemcpyDeviceToHost));
                    if (frames_file) frames_file_ok = frames_file_ok && fwrite(last_pano.data(), 1, last_pano.size(), frames_file) == last_pano.size();
                }
                }
                ++consumed;
                free_slots.push(s);
            }
        });

        std::thread recalibrater;
        std::atomic<int> recalibrations{0};
        std::vector<int> view_round(o.views, 0);          // the round whose mesh each view holds (read after the thread is joined)
        std::atomic<int> solver_iterations{0};
        std::atomic<long long> total_keypoints{0}, total_matches{0}, total_inliers{0}, total_temporal{0};
        std::atomic<float> max_disp{0.f};
        std::string recal_failure;
        if (o.solve_mesh)
            // recalibrateMesh (meshwarper.cpp:378-386) with the mesh actually solved: upload the current frames on the recalibration stream,
            // remap them (createMesh's images[idx]), optimise the mesh from matches and hand it to the compositor -- all while the stitcher
            // runs.  The feature front-end is not part of this build: the matches are synthetic (a parallax that drifts from round to round).
            recalibrater = std::thread([&] {
                try {
                    namespace ff = msshim::featurefinder;
                    msshim::MeshWarper mw(o.views, 10, 10, warp_scale, 1.0, 1.0);
                    mw.params().theta_rule = 1;
                    mw.params().global_dist = std::max(4, std::min(30, o.out_w / 128));    // GLOBAL_DIST = 30 is tuned to 1080p views; scaled for small rigs
                    const bool temporal = o.temporal > 0.0;
                    if (temporal) mw.params().alphas[3] = (float)o.temporal;
                    std::vector<ff::ImageFeatures<DevMat>> prev_feats;                          // --temporal: prev_features (meshwarper.cpp:313), device descriptors included
                    std::vector<DevMat> recal_full(o.views), images(o.views);
                    std::vector<ms_view_geom> g(o.views);
                    for (int i = 0; i < o.views; ++i) {
                        g[i] = comp.viewGeom(i);
                        recal_full[i].create(o.h, o.w, MS_8UC3, 3);
                        images[i].create(g[i].roi.height, g[i].roi.width, MS_8UC3, 3);
                    }
                    int round = 1;
                    while (running.load()) {
                        std::this_thread::sleep_for(std::chrono::milliseconds(5));
                        {
                            std::lock_guard<std::mutex> lk(imgs.mu);
                            if (!o.nv12)
                                for (int i = 0; i < o.views; ++i)
                                    HIPCHECK(hipMemcpy2DAsync(recal_full[i].data, recal_full[i].step, imgs.v[i].p, (size_t)o.w * 3, (size_t)o.w * 3, o.h,
                                                              hipMemcpyHostToDevice, recal_stream));
                            HIPCHECK(hipStreamSynchronize(recal_stream));
                        }
                        for (int i = 0; i < o.views; ++i) {
                            ms_image xm, ym;
                            msshim::check(ms_get_maps(comp.raw(), i, &xm, &ym));
                            ms_image src = msshim::wrap(recal_full[i]), dst = msshim::wrap(images[i]);
                            msshim::check(ms_remap(&src, &xm, &ym, &dst, MS_INTER_LINEAR_FIXPT, MS_BORDER_CONSTANT, (ms_stream)recal_stream));   // cv::remap, meshwarper.cpp:72
                        }
                        // createMesh's front-end (meshwarper.cpp:82-119), all on the device: overlap masks, ORB, Hamming 2-NN + ratio test, RANSAC homographies
                        std::vector<DevMat> fmasks;
                        ff::featureMasks(images, fmasks, std::min(400, std::max(16, o.out_w / 10)), (ms_stream)recal_stream);
                        std::vector<ff::ImageFeatures<DevMat>> feats;
                        ff::findFeatures(images, fmasks, feats, (ms_stream)recal_stream);
                        std::vector<ff::MatchesInfo> pairwise(o.views);                      // NUM_IMAGES - 1 + wrapAround (calibration.cpp:284)
                        std::vector<ff::MatchesInfo> temporal_matches(temporal ? o.views : 0);
                        if (temporal && !prev_feats.empty()) ff::matchFeaturesBoth(feats, prev_feats, pairwise, temporal_matches, (ms_stream)recal_stream);
                        else ff::matchFeatures(feats, pairwise, (ms_stream)recal_stream);
                        for (auto &m : fmasks) if (m.data) HIPCHECK(hipFree(m.data));
                        if (!temporal) for (auto &f : feats) if (f.descriptors.data) HIPCHECK(hipFree(f.descriptors.data));
                        for (auto &f : prev_feats) if (f.descriptors.data) HIPCHECK(hipFree(f.descriptors.data));      // the round before: matched, not needed again
                        { size_t nk = 0, nm = 0, ni = 0; for (auto &f : feats) nk += f.keypoints.size(); for (auto &pm : pairwise) { nm += pm.matches.size(); ni += pm.num_inliers; }
                          total_keypoints += (long long)nk; total_matches += (long long)nm; total_inliers += (long long)ni; }
                        const ms_mesh_info info = temporal ? mw.calibrateMeshWarp(comp, images, feats, pairwise, temporal_matches, prev_feats, (ms_stream)recal_stream)
                                                           : mw.calibrateMeshWarp(comp, images, feats, pairwise, (ms_stream)recal_stream);
                        if (temporal) { total_temporal += (long long)mw.temporalSelected(); prev_feats = feats; }      // (DevMat copies are handles: the descriptors stay where they are)
                        solver_iterations += info.iterations;
                        if (getenv("STITCH_APP_TRACE")) {
                            size_t nm = 0; for (auto &pm : pairwise) nm += pm.matches.size();
                            fprintf(stderr, "round %d: matches %zu rows %d nnz %d iterations %d error %.3g\n", round, nm, info.rows, info.nnz, info.iterations, info.error);
                        }
                        for (int i = 0; i < o.views; ++i) {
                            float dpx = 0.f;
                            msshim::check(ms_get_mesh_displacement(comp.raw(), i, &dpx));
                            if (dpx > max_disp.load()) max_disp.store(dpx);
                        }
                        ++round; ++recalibrations;
                    }
                    for (auto &f : prev_feats) if (f.descriptors.data) HIPCHECK(hipFree(f.descriptors.data));
                } catch (const std::exception &e) { recal_failure = e.what(); }
            });
        else if (o.cpw)
            recalibrater = std::thread([&] {            // timed.cpp:414-463: new meshes while the stitcher keeps running
                int round = 1;
                while (running.load()) {
                    std::this_thread::sleep_for(std::chrono::milliseconds(5));
                    for (int i = 0; i < o.views && running.load(); ++i) {
                        const ms_view_geom g = comp.viewGeom(i);
                        std::vector<float> mx, my;
                        make_mesh(g.roi.width, g.roi.height, 10, 10, 0.1 * i + 0.37 * round, 6.0, mx, my);
                        comp.convertMeshToMap(i, mx.data(), my.data(), 10, 10, recal_stream);
                        if (o.update_mask > 0) comp.update_mask(i, (ms_stream)recal_stream);      // timed.cpp:598-605
                        view_round[i] = round;
                    }
                    ++round; ++recalibrations;
                }
            });

        const auto t0 = std::chrono::steady_clock::now();
        std::string failure;
        const unsigned all_views = (1u << o.views) - 1u;
        unsigned active_views = all_views;
        long long degraded_frames = 0;
        try {
        for (int t = 0; t < o.frames; ++t) {            // main loop: stitch_one per frame
            Slot *s = free_slots.pop();
            if (o.drop_view >= 0) {     // capture timeout: the cameras that have not delivered frame t within CAMERA_TIMEOUT_MS are left out of it
                stitch_frame.store(t);
                const auto deadline = std::chrono::steady_clock::now() + std::chrono::milliseconds(CAMERA_TIMEOUT_MS);
                unsigned fresh = 0;
                for (;;) {
                    fresh = 0;
                    { std::lock_guard<std::mutex> lk(imgs.mu); for (int i = 0; i < o.views; ++i) if (imgs.v[i].seq >= t) fresh |= 1u << i; }
                    if (fresh == all_views || std::chrono::steady_clock::now() >= deadline) break;
                    std::this_thread::sleep_for(std::chrono::microseconds(50));
                }
                if (fresh == 0) fresh = active_views;      // (no camera at all: keep the last set)
                if (fresh != active_views) { comp.setActiveViews(fresh, (ms_stream)stitch_stream); active_views = fresh; }      // enqueue-only
                degraded_frames += active_views != all_views;
            }
            const int ib = o.upload ? (t & 1) : 0;
            std::vector<DevMat> &full_imgs = full_imgs_b[ib], &nv12_imgs = nv12_imgs_b[ib];
            const bool ramp_now = o.ramp_view >= 0 && t == o.frames / 2;
            if (ramp_now) {                         // --exposure-ramp: camera V's exposure changes here
                std::lock_guard<std::mutex> lk(imgs.mu);
                HIPCHECK(hipStreamSynchronize(upload_stream));                            // (no copy still reads the pinned frame)
                unsigned char *p = imgs.v[o.ramp_view].p;
                const size_t ramp_bytes = o.nv12 ? (size_t)o.w * o.h : host_frame_bytes;      // NV12: the Y plane only
                for (size_t i = 0; i < ramp_bytes; ++i) p[i] = (unsigned char)std::min(255.0, std::floor(p[i] * o.ramp_factor + 0.5));
            }
            if (o.upload || t == 0 || ramp_now) {
                std::lock_guard<std::mutex> lk(imgs.mu);                                  // imgs.lock() ... imgs.unlock()
                if (buf_used[ib]) HIPCHECK(hipStreamWaitEvent(upload_stream, buf_free[ib], 0));     // the stitch of frame t-2 has read this buffer
                if (o.nv12)               // half the PCIe bytes: upload NV12 (all cameras in one copy), convert on the device / in the warp
                    HIPCHECK(hipMemcpyAsync(nv12_imgs[0].data, host_slab, host_frame_bytes * o.views, hipMemcpyHostToDevice, upload_stream));
                else                      // GpuMat::upload(Mat, stream) of every camera (timed.cpp:68), as one copy
                    HIPCHECK(hipMemcpyAsync(full_imgs[0].data, host_slab, host_frame_bytes * o.views, hipMemcpyHostToDevice, upload_stream));
                HIPCHECK(hipEventRecord(up_done[ib], upload_stream));
                HIPCHECK(hipStreamWaitEvent(stitch_stream, up_done[ib], 0));
                if (o.nv12 && !(o.nv12_direct && !resize_in) && !fused_resize) {             // cvtColor(YUV2BGR_NV12) of all cameras in one launch (also with --nv12-direct when the frames are resized first: the resize works on BGR) (the reference: per camera, on the CPU, networking.cpp:45-47).
                                          // On the STITCH stream (round 4): the upload stream then carries nothing but the copies, so the PCIe link -- the limit of
                                          // this path -- never waits for a kernel; the conversion (one latency-bound launch) rides in front of the frame's stitch
                    std::vector<ms_image> a(o.views), d(o.views);
                    for (int i = 0; i < o.views; ++i) { a[i] = msshim::wrap(nv12_imgs[i]); d[i] = msshim::wrap(full_imgs[i]); }
                    msshim::check(ms_nv12_to_bgr_batch(a.data(), d.data(), o.views, (ms_stream)stitch_stream));
                }
            }
            if (resize_in) {                        // timed.cpp:75-85: cuda::resize(full_imgs[i], resized, Size(), compose_scale, compose_scale)
                if (fused_resize) msshim::cuda::resize_nv12(nv12_imgs, small_imgs, cal.rig.compose_scale, cal.rig.compose_scale, (ms_stream)stitch_stream);      // planes -> small_imgs, one pass
                else msshim::cuda::resize(full_imgs, small_imgs, cal.rig.compose_scale, cal.rig.compose_scale, (ms_stream)stitch_stream);      // all views, one launch
                comp.stitch_one(small_imgs, &s->pano8u, (DevMat *)nullptr, (ms_stream)stitch_stream);
            } else if (nv12_i420) {        // planes in, planes out: neither BGR frames nor a BGR canvas
                std::vector<DevMat> planes(1, s->i420);
                comp.stitch_one_nv12_i420(nv12_imgs, planes, (ms_stream)stitch_stream);
            } else if (o.nv12_direct)      // (resize_in is false here)
                comp.stitch_one_nv12(nv12_imgs, &s->pano8u, (DevMat *)nullptr, (ms_stream)stitch_stream);      // the warp converts each tap itself: no BGR frames on the device at all
            else
                comp.stitch_one(full_imgs, &s->pano8u, (DevMat *)nullptr, (ms_stream)stitch_stream);
            if (o.track_gains > 0 && (t + 1) % o.track_gains == 0) {    // exposure tracking: enqueue-only, behind the stitch that read the same frames
                if (o.nv12_direct && !resize_in) comp.trackGainsNv12(nv12_imgs, 0, 0, (ms_stream)stitch_stream);      // (no BGR frames exist)
                else comp.trackGains(resize_in ? small_imgs : full_imgs, 0, 0, (ms_stream)stitch_stream);
            }
            if (o.i420 && !nv12_i420) {
                ms_image rows{s->pano8u.data + (size_t)ya * s->pano8u.step, s->pano8u.step, o.out_w, yb - ya, MS_8UC3};
                ms_image dst = msshim::wrap(s->i420);
                msshim::check(ms_bgr_to_i420(&rows, &dst, (ms_stream)stitch_stream));       // cvtColor(BGR2YUV_I420), timed.cpp:308-316
            }
            s->seq = t;
            HIPCHECK(hipEventRecord(s->done, stitch_stream));
            HIPCHECK(hipEventRecord(buf_free[ib], stitch_stream)); buf_used[ib] = true;
            results.push(s);
        }
        } catch (const msshim::Error &e) { failure = e.what(); }        // threads must be joined before the error is reported
        results.push(nullptr);
        consumer.join();
        const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        running.store(false);
        capture.join();
        if (recalibrater.joinable()) recalibrater.join();
        HIPCHECK(hipDeviceSynchronize());
        if (frames_file) { frames_file_ok = fclose(frames_file) == 0 && frames_file_ok; if (!frames_file_ok) { fprintf(stderr, "cannot write %s\n", o.dump_frames.c_str()); return 2; } }
        if (!failure.empty()) { fprintf(stderr, "stitch_app: %s\n", failure.c_str()); return 1; }
        if (!recal_failure.empty()) { fprintf(stderr, "stitch_app (recalibration): %s\n", recal_failure.c_str()); return 1; }

        // --update-mask self-check: whatever interleaving of stitches, mesh swaps and enqueue-only mask updates happened above, the tables the context ended
        // up with must be exactly what a fresh context gets from the same final meshes with the synchronous update_mask (one more frame through both)
        int selfcheck = -1;
        if (o.update_mask > 0 && !o.solve_mesh && !o.reference_calib) {
            msshim::Compositor ref(o.views, o.w, o.h, MS_PROJ_SPHERICAL, (float)(o.out_w / (2.0 * M_PI)), o.bands, true, o.out_w, o.out_h, 1, 0);
            for (int i = 0; i < o.views; ++i) {
                ref.setCamera(i, cal.rig.K_compose[i], cal.rig.R[i]);
                ref.setGain(i, 1.0 + 0.02 * (i - (o.views - 1) / 2.0));
            }
            ref.buildMaps(); ref.buildMasks(true); ref.init_gpu();
            std::vector<DevMat> views(o.views);
            std::vector<unsigned char> host((size_t)o.w * o.h * 3);
            for (int i = 0; i < o.views; ++i) {
                const ms_view_geom g = ref.viewGeom(i);
                std::vector<float> mx, my;
                make_mesh(g.roi.width, g.roi.height, 10, 10, 0.1 * i + (view_round[i] ? 0.37 * view_round[i] : 0.0), 6.0, mx, my);
                ref.convertMeshToMap(i, mx.data(), my.data(), 10, 10, nullptr);
                views[i].create(o.h, o.w, MS_8UC3, 3);
                synth_frame(host.data(), o.w, o.h, (i + 3) % o.views);
                HIPCHECK(hipMemcpy2D(views[i].data, views[i].step, host.data(), (size_t)o.w * 3, (size_t)o.w * 3, o.h, hipMemcpyHostToDevice));
            }
            for (int i = 0; i < o.views; ++i)
                if (view_round[i]) ref.update_mask(i, nullptr);          // (round 0 = the start-up meshes: no mask update was issued for them)
            DevMat a, b;
            a.create(o.out_h, o.out_w, MS_8UC3, 3); b.create(o.out_h, o.out_w, MS_8UC3, 3);
            HIPCHECK(hipMemset2D(a.data, a.step, 0, (size_t)o.out_w * 3, o.out_h)); HIPCHECK(hipMemset2D(b.data, b.step, 0, (size_t)o.out_w * 3, o.out_h));
            comp.stitch_one(views, &a, (DevMat *)nullptr, (ms_stream)stitch_stream);
            ref.stitch_one(views, &b, (DevMat *)nullptr, nullptr);
            HIPCHECK(hipDeviceSynchronize());
            std::vector<unsigned char> ha((size_t)o.out_w * o.out_h * 3), hb(ha.size());
            HIPCHECK(hipMemcpy2D(ha.data(), (size_t)o.out_w * 3, a.data, a.step, (size_t)o.out_w * 3, o.out_h, hipMemcpyDeviceToHost));
            HIPCHECK(hipMemcpy2D(hb.data(), (size_t)o.out_w * 3, b.data, b.step, (size_t)o.out_w * 3, o.out_h, hipMemcpyDeviceToHost));
            selfcheck = ha == hb ? 1 : 0;
            for (auto &m : views) HIPCHECK(hipFree(m.data));
            HIPCHECK(hipFree(a.data)); HIPCHECK(hipFree(b.data));
        }
        for (unsigned char b : last_pano) checksum = (checksum ^ b) * 1099511628211ull;   // FNV-1a over the last 8U panorama
        if (!o.dump_i420.empty()) {
            FILE *f = fopen(o.dump_i420.c_str(), "wb");
            if (!f || fwrite(last_i420.data(), 1, last_i420.size(), f) != last_i420.size()) { fprintf(stderr, "cannot write %s\n", o.dump_i420.c_str()); return 2; }
            fclose(f);
        }
        if (!o.dump.empty()) {
            FILE *f = fopen(o.dump.c_str(), "wb");
            if (!f || fwrite(last_pano.data(), 1, last_pano.size(), f) != last_pano.size()) { fprintf(stderr, "cannot write %s\n", o.dump.c_str()); return 2; }
            fclose(f);
        }
        printf("{\"app\": \"stitch_app\", \"views\": %d, \"src\": \"%dx%d\", \"out\": \"%dx%d\", \"bands\": %d, \"cpw\": %s, \"i420\": %s, \"nv12\": %s, \"nv12_direct\": %s, \"upload\": %s, "
               "\"frames\": %lld, \"seconds\": %.4f, \"frames_per_s\": %.1f, \"recalibrations\": %d, \"mesh_solver_iterations\": %d, \"max_mesh_displacement_px\": %.2f, "
               "\"orb_keypoints\": %lld, \"ratio_matches\": %lld, \"ransac_inliers\": %lld, \"update_mask_margin\": %d, \"update_mask_equals_sync_rebuild\": %s, \"consume_image_height\": %d, \"consume_checksum\": \"%016llx\", \"checksum\": \"%016llx\", \"degraded_frames\": %lld, \"i420_call\": \"%s\", \"fused_resize\": %s, \"map_source\": %d, \"seam_finder\": \"%s\"",
               o.views, o.w, o.h, o.out_w, o.out_h, pg.num_bands, o.cpw ? "true" : "false", o.i420 ? "true" : "false", o.nv12 ? "true" : "false", o.nv12_direct ? "true" : "false", o.upload ? "true" : "false",
               consumed, secs, consumed / secs, recalibrations.load(), solver_iterations.load(), (double)max_disp.load(),
               total_keypoints.load(), total_matches.load(), total_inliers.load(), o.update_mask, selfcheck < 0 ? "null" : (selfcheck ? "true" : "false"), consume_image_height, consume_checksum, checksum, degraded_frames, i420_call, fused_resize ? "true" : "false", comp.mapSource(), comp.seamFinder() == MS_SEAM_DP ? "dp" : "voronoi");
        if (view_on) printf(", \"view_out\": \"%dx%d\", \"view_checksum\": \"%016llx\"", view_w, view_h, view_checksum);
        if (o.aa) printf(", \"aa_levels\": %d", o.aa);
        if (o.orbit) printf(", \"orbit_deg\": %g", o.orbit_deg);
        if (o.temporal > 0.0) printf(", \"temporal_alpha\": %g, \"temporal_matches\": %lld", o.temporal, total_temporal.load());
        if (o.track_gains > 0) {
            std::vector<double> g((size_t)o.views);
            int ok = 0, singular = 0;
            msshim::check(ms_get_gains(comp.raw(), g.data(), &ok, &singular, (ms_stream)stitch_stream));
            printf(", \"track_gains\": %d, \"gain_solves_ok\": %d, \"gain_solves_singular\": %d, \"gains\": [", o.track_gains, ok, singular);
            for (int i = 0; i < o.views; ++i) printf("%s%.9g", i ? ", " : "", g[i]);
            printf("]");
        }
        printf("}\n");
        if (o.drop_view >= 0) fprintf(stderr, "stitch_app: %lld of %lld frames stitched without every camera\n", degraded_frames, consumed);
    } catch (const msshim::Error &e) {
        fprintf(stderr, "stitch_app: msstitch error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
