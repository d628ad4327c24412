"""ms_create_mesh's fp64 least-squares CG (k_lscg_step / k_lscg_cols, csrc/mesh_solver.hip) where test_mesh_solver_gpu.py does not reach:

1. Systems past the grid caps.  Both kernels launch on at most LSCG_PARTS = 512 workgroups: k_lscg_cols (16 lanes per column) strides its
   column loop once the system has more than 512 * 16 = 8192 unknowns, k_lscg_step strides its row and column loops past 512 * 256 = 131072
   rows, and sum_parts then consumes all 512 partials.  Three shapes: 36 x 36 on 6 views of 150 x 110 (133296 x 15552: both caps, the
   smallest such case), 17 x 17 on 16 views of 90 x 60 (75168 x 9248: only k_lscg_cols strides) and 40 x 40 on 6 views of 333 x 207
   (165360 x 19200: the mesh and view count of the benchmarked configuration).  Each is checked against the oracle's restated Eigen loop
   (1e-3 px, the module's contract) and against a sparse direct solve of the normal equations, which shares nothing with either CG.
   k_lscg_step's loop over the unknowns strides only past 131072 of them (65536 vertices): 105 x 105 on 6 views of 210 x 210, 132300
   unknowns, with the smoothness term weighted 0 because the oracle's costs seconds per 10 000 vertices.

2. Iteration caps at the edges of the host's launch blocks (LSCG_BLOCK = 64 iterations per look at the convergence flag): caps 1, 2, 3
   (both parities of the p buffers and abs_new slots) and 63, 64, 65, 128, 129.  Here the iterate is pinned to the last float32 bit: the
   bound is half a float32 ulp of the oracle's value (the float64 -> float32 store) plus 16 x s_k, where s_k is how far the oracle moves
   when only the order of its own sums changes (the system's rows permuted).  Measured: s_k <= 1.2e-13 px for k <= 65, <= 3e-11 px for
   k <= 129, next to a float32 half-ulp of 3.8e-6 px and a last CG step of 47 px (k = 1) down to 2.9e-3 px (k = 128).

3. No dependence on what an earlier, larger call left in the per-thread device scratch.

The oracle's systems are assembled once per module and only read."""
import functools

import numpy as np
import pytest

import mesh_oracle as mo
from helpers import host, to_dev
from test_mesh_oracle import rig

pytestmark = pytest.mark.gpu

COLS_CAP = 512 * 16             # k_lscg_cols: LSCG_PARTS workgroups, 16 columns each
ROWS_CAP = 512 * 256            # k_lscg_step: LSCG_PARTS workgroups, 256 rows each

#        name                    views  view size   mesh  rows > ROWS_CAP
CAPPED = {"both_caps_36x36": (6, 150, 110, 36, True),
          "cols_cap_only_17x17": (16, 90, 60, 17, False),
          "benchmarked_40x40": (6, 333, 207, 40, True)}


def theta(n):
    return lambda s, d: mo.generic_theta(s, d, n)


@functools.lru_cache(maxsize=None)
def capped_inputs(name):
    n, w, h, M, _ = CAPPED[name]
    images, matches = rig(n=n, seed=12, w=w, h=h)
    return images, matches


@functools.lru_cache(maxsize=None)
def capped_oracle(name):
    """The oracle's system, its LSCG answer and the direct answer; computed once, read by the tests."""
    import scipy.sparse.linalg as spla
    n, w, h, M, _ = CAPPED[name]
    images, matches = capped_inputs(name)
    S = mo.assemble(images, matches, M, M, focal=60.0, global_dist=8, theta_fn=theta(n))
    A, b = S.csr()
    x, it, err = mo.lscg(A, b)
    direct = spla.spsolve((A.T @ A).tocsc(), A.T @ b)
    return dict(rows=S.rows, cols=S.cols, nnz=len(S.v), x=x, iterations=it, error=err, direct=direct)


def capped_solve(ms, name):
    n, w, h, M, _ = CAPPED[name]
    images, matches = capped_inputs(name)
    prm = ms.mesh_default_params(mesh_cols=M, mesh_rows=M, focal_length=60.0, theta_rule=1, global_dist=8)
    return ms.create_mesh([to_dev(im) for im in images], matches, prm)


def same_bytes(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]


@pytest.mark.parametrize("name", list(CAPPED))
def test_capped_grids_match_oracle_and_direct_solve(ms, cuda, name):
    """Measured on an MI355X: in all three cases every float32 vertex equals the oracle's and the direct solve's (both gaps 0 px);
    iterations device / oracle 496 / 496, 497 / 497 and 440 / 446; error 2.14e-16, 2.05e-16 and 2.08e-16 (oracle 2.17e-16, 2.07e-16, 2.21e-16)."""
    n, w, h, M, rows_capped = CAPPED[name]
    ref = capped_oracle(name)
    mx, my, info = capped_solve(ms, name)
    assert (info["rows"], info["cols"], info["nnz"]) == (ref["rows"], ref["cols"], ref["nnz"])
    # the premise: these systems leave the one-element-per-thread regime (a larger LSCG_PARTS must not quietly turn them into small cases)
    assert info["cols"] > COLS_CAP
    assert (info["rows"] > ROWS_CAP) == rows_capped
    rx, ry = mo.vector_to_mesh(ref["x"], n, M, M)
    dx, dy = mo.vector_to_mesh(ref["direct"], n, M, M)
    gap_o = max(np.abs(mx - rx).max(), np.abs(my - ry).max())
    gap_d = max(np.abs(mx - dx).max(), np.abs(my - dy).max())
    print("\n%s: %d x %d, |device - oracle| %.3g px, |device - direct| %.3g px, iterations %d / %d, error %.3g / %.3g"
          % (name, info["rows"], info["cols"], gap_o, gap_d, info["iterations"], ref["iterations"], info["error"], ref["error"]))
    assert gap_o < 1e-3
    assert gap_d < 1e-3
    assert abs(info["iterations"] - ref["iterations"]) <= max(3, ref["iterations"] // 50) and info["error"] < 2.3e-16
    # the matches do move the mesh
    gx = np.array([j * w // (M - 1) for j in range(M)], np.float32)
    assert np.abs(mx - gx[None, None, :]).max() > 1.0
    # fixed-order reductions over all 512 partials: reproducible bit for bit
    assert same_bytes((mx, my, info), capped_solve(ms, name))


@functools.lru_cache(maxsize=None)
def wide_system():
    """More unknowns than k_lscg_step has threads (105 x 105 on 6 views of 210 x 210: 132300 > 131072).  The oracle's smoothness term costs
    seconds per 10 000 vertices, so this system has none: smoothness weight 0 (the device still emits those rows, with every coefficient 0, and
    still counts them) and GLOBAL_DIST 0, which pins every vertex and keeps the normal equations regular.  What is left, the oracle's local and
    global terms, couples the views through the matches: the oracle's CG needs 284 iterations."""
    import scipy.sparse.linalg as spla
    n, w, h, M = 6, 210, 210, 105
    images, matches = rig(n=n, seed=12, w=w, h=h)
    alphas = (1.0, 0.01, 0.0, 0.0)
    S = mo.System(n, M, M)
    for idx in range(n):                    # mo.assemble without the smoothness term (whose rows are all zero at weight 0)
        mo.local_term(S, matches[idx], [(w, h)] * n, idx, alphas[0], 60.0, 1.0, 1.0, theta(n))
        mo.global_term(S, [(mo.cv_round(m[0]), mo.cv_round(m[1])) for m in matches[idx]], (w, h), idx, alphas[1], 0)
    A, b = S.csr()
    x, it, err = mo.lscg(A, b)
    direct = spla.spsolve((A.T @ A).tocsc(), A.T @ b)
    # (vertex, triangle) pairs that stay inside the mesh: per triangle, the vertices whose three offsets all do
    triangles = sum((M - max(dx for dx, _ in tri) + min(dx for dx, _ in tri)) * (M - max(dy for _, dy in tri) + min(dy for _, dy in tri)) for tri in mo.TRIANGLES)
    return dict(n=n, w=w, M=M, images=images, matches=matches, alphas=alphas, x=x, iterations=it, error=err, direct=direct,
                rows=S.rows + 2 * n * triangles, cols=S.cols, nnz=len(S.v) + 12 * n * triangles)


def test_more_unknowns_than_step_threads(ms, cuda):
    """k_lscg_step's loop over the unknowns (x += alpha p, p' = z + beta p) strides only past 512 * 256 unknowns.  Against the oracle's CG and
    the direct solve of the same system.  Measured on an MI355X: 1170780 x 132300, both gaps 0 px, 284 iterations on either side, error 1.9e-16
    (oracle 2.17e-16)."""
    ref = wide_system()
    n, M = ref["n"], ref["M"]
    prm = ms.mesh_default_params(mesh_cols=M, mesh_rows=M, focal_length=60.0, theta_rule=1, global_dist=0, alphas=ref["alphas"])
    views = [to_dev(im) for im in ref["images"]]
    mx, my, info = ms.create_mesh(views, ref["matches"], prm)
    assert (info["rows"], info["cols"], info["nnz"]) == (ref["rows"], ref["cols"], ref["nnz"])
    assert info["cols"] > ROWS_CAP
    rx, ry = mo.vector_to_mesh(ref["x"], n, M, M)
    dx, dy = mo.vector_to_mesh(ref["direct"], n, M, M)
    gap_o = max(np.abs(mx - rx).max(), np.abs(my - ry).max())
    gap_d = max(np.abs(mx - dx).max(), np.abs(my - dy).max())
    print("\nwide: %d x %d, |device - oracle| %.3g px, |device - direct| %.3g px, iterations %d / %d, error %.3g / %.3g"
          % (info["rows"], info["cols"], gap_o, gap_d, info["iterations"], ref["iterations"], info["error"], ref["error"]))
    assert gap_o < 1e-3
    assert gap_d < 1e-3
    assert abs(info["iterations"] - ref["iterations"]) <= max(3, ref["iterations"] // 50) and info["error"] < 2.3e-16
    # the matches move the mesh; the unknowns past the loop's first pass (the last rows of the last view) end far from the 0 they start at
    gx = np.array([j * ref["w"] // (M - 1) for j in range(M)], np.float32)
    assert np.abs(mx - gx[None, None, :]).max() > 1.0
    tail = slice((ROWS_CAP // 2) - (n - 1) * M * M, None)          # vertices of the last view whose unknowns are 131072 and up
    assert np.abs(rx[-1].ravel()[tail]).max() > 100.0
    assert same_bytes((mx, my, info), ms.create_mesh(views, ref["matches"], prm))

# ------------------------------------------------------------------------------------------------ iteration caps at the launch-block edges

BLOCK_EDGE_CAPS = (1, 2, 3, 63, 64, 65, 128, 129)       # not 192 or beyond: there the oracle differs from itself by 5e-6 px


@functools.lru_cache(maxsize=None)
def block_edge_system():
    """The 10 x 10, 6-view system (1200 unknowns; the oracle converges in 465 iterations, so every cap is reached) and four row permutations."""
    images, matches = rig(n=6, seed=2)
    A, b = mo.assemble(images, matches, 10, 10, focal=60.0, global_dist=8, theta_fn=theta(6)).csr()
    perms = [np.random.default_rng(100 + i).permutation(A.shape[0]) for i in range(4)]
    return images, matches, A, b, [(A[p], b[p]) for p in perms]


def ulp32(x):
    """The float32 spacing at |x| (x in float64, normal range)."""
    ax = np.abs(x)
    return np.where(ax > 0, np.ldexp(1.0, np.frexp(ax)[1] - 24), 0.0)


@pytest.mark.parametrize("k", BLOCK_EDGE_CAPS)
def test_iteration_caps_at_launch_block_edges(ms, cuda, k):
    """The iterate after exactly k iterations, to the last float32 bit: |float64(v) - x_ref| <= ulp32(x_ref) / 2 + 16 s_k, with s_k the largest
    difference between the oracle's iterates over the system's rows in five orders (as assembled and four permutations): what the order of the
    sums alone does to the reference.  16: the device's tree-shaped sums against numpy's sequential ones.  info["error"] relatively, within
    16 x the oracle's own relative spread over the same orders (floor 1e-12).  And the test could fail: the oracle's iterates k - 1 and k
    differ by more than 100 x the bound, so one update too few or too many cannot pass.

    Measured (CPU oracle; device on an MI355X).  The gap is the float32 store's: at every k all 1200 device values equal float32(oracle's).
         k    s_k [px]   error spread   step k-1 -> k [px]   max bound [px]   max |device - oracle| [px]   error gap (relative)
         1    5.7e-14    9.1e-16        46.6                 1.907e-06        1.851e-06                    0
         2    2.8e-14    6.8e-16        26.1                 1.907e-06        1.898e-06                    3.4e-16
         3    2.8e-14    7.6e-16        16.0                 1.907e-06        1.890e-06                    5.0e-16
        63    1.1e-13    3.3e-15        0.307                3.815e-06        3.685e-06                    2.9e-15
        64    1.1e-13    3.5e-15        0.295                3.815e-06        3.803e-06                    2.3e-15
        65    1.1e-13    3.9e-15        0.252                3.815e-06        3.793e-06                    2.0e-15
       128    2.1e-11    1.0e-09        0.00293              3.815e-06        3.812e-06                    2.9e-10
       129    2.9e-11    2.8e-10        0.00325              3.815e-06        3.809e-06                    4.4e-10"""
    images, matches, A, b, permuted = block_edge_system()
    x, it, err = mo.lscg(A, b, max_iterations=k)
    assert it == k
    runs = [mo.lscg(Ap, bp, max_iterations=k) for Ap, bp in permuted]
    xs = np.array([x] + [r[0] for r in runs])
    errs = np.array([err] + [r[2] for r in runs])
    s_k = float((xs.max(0) - xs.min(0)).max())
    err_spread = float((errs.max() - errs.min()) / err)
    bound = ulp32(x) / 2 + 16 * s_k
    x_prev = mo.lscg(A, b, max_iterations=k - 1)[0] if k > 1 else np.zeros_like(x)        # (max_iterations = 0 means Eigen's default cap)
    step = float(np.abs(x - x_prev).max())
    assert step > 100 * bound.max(), (step, bound.max())

    prm = ms.mesh_default_params(mesh_cols=10, mesh_rows=10, focal_length=60.0, theta_rule=1, global_dist=8, max_iterations=k)
    mx, my, info = ms.create_mesh([to_dev(im) for im in images], matches, prm)
    got = np.stack([mx, my], -1).astype(np.float64).ravel()
    gap = np.abs(got - x)
    err_gap = abs(info["error"] - err) / err
    other_bits = int((got.astype(np.float32) != x.astype(np.float32)).sum())      # (a value the oracle puts within s_k of a rounding tie may fall either way)
    print("\nk %3d  s_k %.3g  error spread %.3g  step %.3g  max bound %.4g  max gap %.4g  worst gap/bound %.3f  error gap %.3g  float32 values unlike the oracle's %d"
          % (k, s_k, err_spread, step, bound.max(), gap.max(), (gap / bound).max(), err_gap, other_bits))
    assert info["iterations"] == k
    assert (gap <= bound).all(), (gap.max(), (gap / bound).max())
    assert err_gap <= max(16 * err_spread, 1e-12), (info["error"], err, err_spread)


# ------------------------------------------------------------------------------------------------ stale scratch

def test_small_solve_is_the_same_after_a_large_one(ms, cuda):
    """The device scratch is a per-thread grow-only block of which the solver zeroes tmp, x and the p buffers only: z and the partial-sum
    arrays of a small system land on whatever a larger one left there.  The 6 x 5, 3-view system (full solve and capped at 9 iterations)
    before and after the 36 x 36 one: identical bytes, info included."""
    images, matches = rig(n=3, seed=7)
    views = [to_dev(im) for im in images]

    def small():
        out = []
        for cap in (0, 9):
            prm = ms.mesh_default_params(mesh_cols=6, mesh_rows=5, focal_length=60.0, theta_rule=1, max_iterations=cap, global_dist=8)
            out.append(ms.create_mesh(views, matches, prm))
        return out

    before = small()
    _, _, big = capped_solve(ms, "both_caps_36x36")
    assert big["cols"] > COLS_CAP and big["rows"] > ROWS_CAP and big["error"] < 2.3e-16
    after = small()
    assert before[0][2]["iterations"] > 9 and before[1][2]["iterations"] == 9
    for a, c in zip(before, after):
        assert same_bytes(a, c), (a[2], c[2])


def test_small_saliency_is_the_same_after_a_large_one(ms, cuda):
    rng = np.random.default_rng(5)
    small = to_dev(rng.integers(0, 256, (60, 90, 3), dtype=np.uint8))
    large = to_dev(rng.integers(0, 256, (207, 333, 3), dtype=np.uint8))
    before = ms.mesh_saliency(small, 6, 5)
    big = ms.mesh_saliency(large, 40, 40)
    after = ms.mesh_saliency(small, 6, 5)
    assert np.isfinite(big).sum() > np.isfinite(before).sum() > 0
    assert before.tobytes() == after.tobytes()
    assert np.array_equal(before, mo.saliency(host(small), 6, 5), equal_nan=True)
