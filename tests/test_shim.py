"""The C++ drop-in (include/vr/offscreen_pass_hip.hpp) against the reference's call shapes.

tests/shim/reference_call_shapes.cpp holds the reference's OffscreenPass call sites
(vulkan_context.cpp:51, main_pass.cpp:91, imgui_context.cpp:55-75, importer.cpp:41-46,
main_window.cpp:233-238 and :253-257) with stand-in Vulkan/glm/Application types.  CPU: it
compiles and links against lib/libvr_amd.so.  GPU: the program drives two MainPass::render
frames and checks the presenter received exactly vr_render's pixels for the same camera."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "volumetric-renderer_amd", "lib")
SRC = os.path.join(ROOT, "tests", "shim", "reference_call_shapes.cpp")
EXE = os.path.join(LIBDIR, "reference_call_shapes")
EXT_SRC = os.path.join(ROOT, "tests", "shim", "external_memory.cpp")
EXT_EXE = os.path.join(LIBDIR, "external_memory")


def build():
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    SRC, "-o", EXE, "-L", LIBDIR, "-lvr_amd", "-Wl,-rpath," + LIBDIR],
                   check=True, capture_output=True, text=True)
    return EXE


def build_external():
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", EXT_SRC,
                    "-o", EXT_EXE, "-L", LIBDIR, "-lvr_amd", "-Wl,-rpath," + LIBDIR,
                    "-L", "/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"],
                   check=True, capture_output=True, text=True)
    return EXT_EXE


def test_reference_call_shapes_compile_and_link():
    assert os.path.exists(build())


@pytest.mark.gpu
@pytest.mark.parametrize("mask", [None, "0x1"])
def test_reference_call_shapes_present_the_hip_frame(gpu, mask):
    """Unchanged call sites; with Traits::device_mask() set the same construction call
    (vulkan_context.cpp:51) yields a multi-device context (vr_create_mask)."""
    exe = EXE if os.path.exists(EXE) else build()
    r = subprocess.run([exe] + (["--device-mask", mask] if mask else []), capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "match=1" in r.stdout and "device_mask=0x1" in r.stdout


@pytest.mark.gpu
def test_u8_scan_as_float_dataset_is_stored_native(gpu):
    """SURVEY.md §8f-1 / VERDICT r2: the reference's loader makes every voxel a float
    (nrrd_file_parser.cpp:49-77), so an 8-bit scan arrives at volume_dataset_changed as a
    float Dataset.  Through the unchanged import call it is stored as 8-bit voxels (an
    `unsigned char` march kernel), and the presented frame equals the native-u8 upload's."""
    exe = EXE if os.path.exists(EXE) else build()
    r = subprocess.run([exe, "--u8-dataset"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "narrow=1" in r.stdout and "match=1" in r.stdout


def test_external_memory_program_compiles_and_links():
    assert os.path.exists(build_external())


@pytest.mark.gpu
@pytest.mark.parametrize("mask", [None, "0x1"])
def test_frame_rendered_into_imported_memory(gpu, mask):
    """SURVEY.md §8f-3 (zero-copy presentation): a shareable allocation exported as a POSIX fd
    (the vkGetMemoryFdKHR stand-in) is imported with vr_import_memory_fd, two frames are rendered
    into it with vr_render_device, and the exporter reads through ITS OWN mapping exactly
    vr_render's bytes for the same camera, with the bytes around the imported range untouched.
    With a device mask the context is a vr_create_mask group, whose frames land on its lowest
    device."""
    exe = EXT_EXE if os.path.exists(EXT_EXE) else build_external()
    r = subprocess.run([exe] + (["--device-mask", mask] if mask else []), capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "match=1" in r.stdout and "guard=1" in r.stdout
    assert "fd_open_after_release=1" in r.stdout  # the caller keeps the fd (vr.h)


def test_shim_takes_the_clip_form_from_glms_configuration(tmp_path):
    """vr_params.depth_zero_to_one (ABI 8) in the shim: glm's GLM_CONFIG_CLIP_CONTROL (fixed at
    glm's first include) selects it; without glm, or in glm's default [-1, 1] form, it is 0 --
    the reference's build (offscreen_pass.cpp:3 defines GLM_FORCE_DEPTH_ZERO_TO_ONE after glm
    came in through offscreen_pass.h:3).  glm is an un-vendored submodule of the reference, so
    its setup.hpp macros are stated here as glm >= 0.9.9 defines them."""
    src = str(tmp_path / "vr_shim_clip.cpp")
    exe = str(tmp_path / "vr_shim_clip")
    body = r"""
#include <vr/offscreen_pass_hip.hpp>
#include <cstdio>
int main() { std::printf("%d\n", (int)Vol::Rendering::Hip::OffscreenPass::host_depth_zero_to_one()); return 0; }
"""
    outs = {}
    for name, pre in (("none", ""),
                      ("glm_no", "#define GLM_CLIP_CONTROL_ZO_BIT (1 << 0)\n#define GLM_CLIP_CONTROL_NO_BIT (1 << 1)\n"
                                 "#define GLM_CLIP_CONTROL_RH_BIT (1 << 3)\n"
                                 "#define GLM_CONFIG_CLIP_CONTROL (GLM_CLIP_CONTROL_RH_BIT | GLM_CLIP_CONTROL_NO_BIT)\n"),
                      ("glm_zo", "#define GLM_CLIP_CONTROL_ZO_BIT (1 << 0)\n#define GLM_CLIP_CONTROL_RH_BIT (1 << 3)\n"
                                 "#define GLM_CONFIG_CLIP_CONTROL (GLM_CLIP_CONTROL_RH_BIT | GLM_CLIP_CONTROL_ZO_BIT)\n")):
        with open(src, "w") as f:
            f.write(pre + body)
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), src],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        r = subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                            "-L", LIBDIR, "-lvr_amd", "-Wl,-rpath," + LIBDIR],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        outs[name] = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip()
    assert outs == {"none": "0", "glm_no": "0", "glm_zo": "1"}
