"""The C-ABI library loads, exports exactly what include/*.h declare, and refuses to compute
without a device (no CPU fallback)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols(header="ms_stitch.h"):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"MS_API\s+[\w\s\*]+?\b(ms_\w+)\s*\(", text)))


def test_header_symbols_are_exported(ms):
    lib = ms.load()
    names = declared_symbols()
    assert len(names) >= 40
    for n in names:
        assert hasattr(lib, n), "libmsstitch.so does not export %s" % n
    assert sorted(ms.EXPORTS) == names, "msstitch.EXPORTS out of sync with include/ms_stitch.h"
    for doc in ("README.md", "DESIGN.md"):      # the count both documents state is the header's
        stated = re.findall(r"(\d+) entry points, each citing", open(os.path.join(ROOT, doc)).read())
        assert stated == [str(len(names))], "%s states %s entry points, include/ms_stitch.h declares %d" % (doc, stated, len(names))
    # the multi-GPU layer (include/ms_dist.h) lives in the same library
    import msdist
    dist_names = declared_symbols("ms_dist.h")
    assert len(dist_names) >= 12 and sorted(os.listdir(os.path.join(ROOT, "include"))) == ["ms_dist.h", "ms_stitch.h"]
    for n in dist_names:
        assert hasattr(lib, n), "libmsstitch.so does not export %s" % n
    assert sorted(msdist.EXPORTS) == dist_names, "msdist.EXPORTS out of sync with include/ms_dist.h"


def test_no_oracle_in_product():
    """The shipped library must not reference the CPU oracle (nor may the python binding import it)."""
    import subprocess
    out = subprocess.run(["nm", "-D", os.path.join(ROOT, "video-stitcher_amd", "libmsstitch.so")], capture_output=True, text=True).stdout
    assert "orc_" not in out
    for f in ("msstitch.py", "msdist.py", "synth.py", "dist_frames.py"):
        src = open(os.path.join(ROOT, "video-stitcher_amd", f)).read()
        assert "oracle" not in src.replace("no oracle", "").lower() or f == "synth.py" and "import oracle" not in src
    for f in os.listdir(os.path.join(ROOT, "video-stitcher_amd", "csrc")):
        src = open(os.path.join(ROOT, "video-stitcher_amd", "csrc", f)).read()
        assert "ms_oracle.h" not in src and "orc_" not in src


def test_compute_without_device_fails_loudly(ms):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; the no-device path is exercised on the CPU-only container")
    lib = ms.load()
    assert lib.ms_device_count() == 0
    ctx = C.c_void_p()
    cfg = ms.Config(C.sizeof(ms.Config), 2, 64, 48, ms.PROJ_SPHERICAL, 50.0, 2, 0, 0, 0, 1)
    rc = lib.ms_create(C.byref(cfg), C.byref(ctx))
    assert rc == -4 and b"no CPU fallback" in lib.ms_last_error()
    buf = (C.c_uint8 * 64)()
    im = ms.Image(C.cast(buf, C.c_void_p), 8, 8, 8, ms.MS_8UC1)
    assert lib.ms_dilate3x3_8u(C.byref(im), C.byref(im), None) == -4
    with pytest.raises(ms.MsError):
        ms.Compositor(2, (64, 48), ms.PROJ_SPHERICAL, 50.0)


def test_status_and_version(ms):
    lib = ms.load()
    assert b"gfx950" in lib.ms_version()
    r = ms.Rect()
    assert lib.ms_warp_roi(7, None, None, C.c_float(1.0), 10, 10, C.byref(r)) == -1
    assert b"ms_warp_roi" in lib.ms_last_error()


def test_shim_meshwarper_selection_state_machine(tmp_path):
    """msshim::MeshWarper (filterMatches + the use-old-features logic of createMesh) against hand-derived expectations; host only."""
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "shim_mw")
    pkg = os.path.join(ROOT, "video-stitcher_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "shim_meshwarper_check.cpp"),
                           "-L" + pkg, "-lmsstitch", "-Wl,-rpath," + pkg, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr


def test_ms_image_layout_matches_the_references_ptrstepsz():
    """ms_image = PtrStepSz<T> {data, step, cols, rows} + type: checked against the reference's own header where it is present."""
    import subprocess
    inc = "/root/reference/sources/modules/core/include"
    if not os.path.isfile(os.path.join(inc, "opencv2", "core", "cuda_types.hpp")):
        _ms_image_layout_matches_the_stored_ptrstepsz_layout()
        return
    exe = os.path.join(ROOT, "video-stitcher_amd", "build", "abi_layout_check")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++11", "-I" + inc, os.path.join(ROOT, "video-stitcher_amd", "shim", "abi_layout_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "layout ok" in out.stdout, out.stdout


def _ms_image_layout_matches_the_stored_ptrstepsz_layout():
    """Where the reference is not present: the offsets its PtrStepSz<uchar> has (tests/golden/ptrstepsz_layout.json, printed by shim/abi_layout_check.cpp) against
    ms_image as include/ms_stitch.h declares it, compiled here."""
    import json
    import subprocess
    import tempfile
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "ptrstepsz_layout.json")))
    src = ('#include <cstddef>\n#include <cstdio>\n#include "ms_stitch.h"\nint main() { ms_image m; std::printf("%zu %zu %zu %zu %zu %zu %zu\\n", offsetof(ms_image, data), '
           'offsetof(ms_image, step), offsetof(ms_image, cols), offsetof(ms_image, rows), offsetof(ms_image, type), sizeof(m.step), sizeof(m.cols)); return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "layout.cpp"), "w") as f:
            f.write(src)
        subprocess.check_call(["g++", "-std=c++11", "-I" + os.path.join(ROOT, "include"), os.path.join(d, "layout.cpp"), "-o", os.path.join(d, "layout")])
        data, step, cols, rows, typ, sz_step, sz_cols = map(int, subprocess.check_output([os.path.join(d, "layout")], text=True).split())
    assert (data, step, cols, rows) == (want["data"], want["step"], want["cols"], want["rows"])
    assert sz_step == want["sizeof_step"] and sz_cols == want["sizeof_cols"] == 4
    assert want["size"] <= typ + 4 and typ >= rows + 4          # PtrStepSz<T> is a prefix of ms_image; `type` follows `rows`


def test_config_struct_size_is_checked(ms):
    """ms_create refuses a config whose struct_size is not this library's sizeof(ms_config) (before it looks for a device)."""
    lib = ms.load()
    cfg = ms.Config(C.sizeof(ms.Config) - 4, 2, 64, 48, ms.PROJ_SPHERICAL, 50.0, 2, 0, 0, 0, 1)
    ctx = C.c_void_p()
    rc = lib.ms_create(C.byref(cfg), C.byref(ctx))
    assert rc != 0 and ctx.value is None
    if lib.ms_device_count() > 0:
        assert rc == -1 and b"struct_size" in lib.ms_last_error()


def test_load_tables_refuses_garbage_before_touching_the_device(ms):
    """ms_load_tables validates magic / layout / checksum on the host: MS_ERR_INVALID (not MS_ERR_NO_DEVICE) without a GPU"""
    lib = ms.load()
    out = C.c_void_p()
    for blob in (b"", b"\0" * 40, b"MSTBL01\0" + b"\1" * 400, b"MSTBL02\0" + b"\1" * 400):
        b = (C.c_uint8 * max(1, len(blob))).from_buffer_copy(blob.ljust(1, b"\0"))
        rc = lib.ms_load_tables(b, C.c_size_t(len(blob)), C.byref(out), None)
        assert rc == -1 and not out.value, (rc, len(blob))      # MS_ERR_INVALID


def test_no_v_ashr_pk_u8_i32_in_the_device_code(tmp_path):
    """gfx950's v_ashr_pk_u8_i32 (two clamp((a >> s), 0, 255) packed into 16 bits) as ROCm 7.2's clang emits it: the v_or3_b32 that assembles the dword assumes the
    result's upper 16 bits are zero, and on MI355X they are not -- round 5's first 8-pixel NV12 kernel wrote stray bits into every third byte (found by
    tests/test_prims_gpu.py::test_nv12_to_bgr on the GPU; csrc/prims.hip nv12_px carries the workaround).  No GPU test can prove the ABSENCE of the pattern in kernels
    whose tests do not happen to saturate, so the shipped code objects are disassembled here: the instruction must not occur anywhere."""
    import shutil
    import subprocess
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    lib = os.path.join(ROOT, "video-stitcher_amd", "libmsstitch.so")
    if not os.path.exists(objdump):
        pytest.skip("no llvm-objdump")
    shutil.copy(lib, tmp_path / "lib.so")
    subprocess.run([objdump, "--offloading", "lib.so"], cwd=tmp_path, capture_output=True, check=True)
    objs = [f for f in os.listdir(tmp_path) if "gfx950" in f]
    assert objs, "no gfx950 code object found in libmsstitch.so"
    n_inst = 0
    for f in objs:
        dis = subprocess.run([objdump, "-d", f], cwd=tmp_path, capture_output=True, text=True, check=True).stdout
        n_inst += dis.count("\tv_")
        assert "v_ashr_pk_u8_i32" not in dis and "v_ashr_pk_i8_i32" not in dis, f
    assert n_inst > 10000      # (the disassembly really is the kernels)


def test_wave_priority_switch_only_in_the_projection_warp(tmp_path):
    """s_setprio (tile_kernels.hpp MS_PRIO_*): measured faster for the projection warp in its aligned shared-offset form and SLOWER for the CPW remaps, the level-0 reduce and the
    NV12 warp (profiles/r05_experiments.txt) -- the shipped code objects carry the instruction in k_warp_s<false, ., ., true> and nowhere else."""
    import re
    import shutil
    import subprocess
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    lib = os.path.join(ROOT, "video-stitcher_amd", "libmsstitch.so")
    if not os.path.exists(objdump):
        pytest.skip("no llvm-objdump")
    shutil.copy(lib, tmp_path / "lib.so")
    subprocess.run([objdump, "--offloading", "lib.so"], cwd=tmp_path, capture_output=True, check=True)
    with_prio = set()
    for f in [f for f in os.listdir(tmp_path) if "gfx950" in f]:
        cur = None
        for line in subprocess.run([objdump, "-d", "-C", f], cwd=tmp_path, capture_output=True, text=True, check=True).stdout.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
            if m:
                cur = m.group(1)
            elif "s_setprio" in line and cur:
                with_prio.add(cur.split("(")[0])
    assert with_prio, "no s_setprio in the shipped kernels: MS_PRIO_WARP lost?"
    assert all(re.match(r"^(void )?ms::k_warp_s<false, \d+, \d+, true>$", k) for k in with_prio), sorted(with_prio)


def test_diagnostic_entry_points_validate_their_arguments(ms):
    """ms_get_plan_stats / ms_get_stitch_kernels (round 5): null arguments are MS_ERR_INVALID, a struct of another size is refused (struct_size convention of ms_config)"""
    lib = ms.load()
    assert lib.ms_get_plan_stats(None, None) == -1 and lib.ms_get_stitch_kernels(None, None, None) == -1
    assert C.sizeof(ms.PlanStats) == 4 * (1 + 3 + 2 + 2 + 8 + 2 + 8)      # the layout include/ms_stitch.h declares
