"""The drop-in seam, proven with the reference's own main(): oracle/Makefile (ref-dropin)
compiles the UNMODIFIED reference src/render.cc against this repo's headers
(compat/opencl_host.h forwards to hip_host.h, `using OpenCLHost = HipHost`) together with
the reference's own console code (info.cc, color.cc, timer.cc) and links libocrt_hip.so in
place of OpenCL (reference src/render.cc:1-13,84-116,
include/opencl_host.h:6-144).

CPU part (needs the reference tree, or what build() made from it under oracle/_ref/): it builds, no strong symbol is
defined both by the reference's objects and by the library (the ODR clash VERDICT r1 found),
and without a GPU it ends like the reference does: `No device found`.
GPU part: the prebuilt binary (oracle/_ref/, travels to the GPU box) renders the golden PGMs.
"""
import hashlib
import os
import subprocess

import pytest

from conftest import ROOT, mesh_file

ORACLE_DIR = os.path.join(ROOT, "oracle")
DROPIN = os.path.join(ORACLE_DIR, "_ref", "ref_render_dropin")
DROPIN_RING = os.path.join(ORACLE_DIR, "_ref", "ref_render_dropin_ring")  # the same main() with OpenCLHost = HipHostRing
LIB = os.path.join(ROOT, "opencl_raytracer_amd", "lib", "libocrt_hip.so")


def _defined(path, dynamic):
    out = subprocess.run(["nm", "-C", "--defined-only"] + (["-D"] if dynamic else []) + [path], capture_output=True,
                         text=True, check=True).stdout
    strong = set()
    for line in out.splitlines():
        parts = line.split(None, 2)
        if len(parts) == 3 and parts[1] in "TDBR":  # strong text / data / bss / read-only definitions
            strong.add(parts[2])
    return strong


@pytest.fixture(scope="module")
def dropin_built():
    import orc

    if not orc.reference_available():
        # what __graft_entry__.build() made under oracle/_ref/ where the reference tree was present
        objs = [os.path.join(ORACLE_DIR, "_ref", "dropin_obj", n) for n in ("render.o", "info.o", "color.o", "timer.o")]
        if all(os.path.exists(p) for p in [DROPIN, DROPIN_RING] + objs):
            return DROPIN
        pytest.skip("needs the reference tree, or oracle/_ref/ref_render_dropin* built from it")
    r = subprocess.run(["make", "-C", ORACLE_DIR, "ref-dropin"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return DROPIN


def test_reference_render_cc_builds_unmodified_against_the_drop_in(dropin_built):
    assert os.access(dropin_built, os.X_OK)
    # the reference's main() really is in there, and it binds the HIP host
    out = subprocess.run(["nm", "-C", dropin_built], capture_output=True, text=True, check=True).stdout
    assert " T main" in out
    assert "HipHost::upload" in out and "HipHost::operator()()" in out
    ring = subprocess.run(["nm", "-C", DROPIN_RING], capture_output=True, text=True, check=True).stdout
    assert " T main" in ring and "HipHostRing::upload" in ring and "HipHostRing::operator()()" in ring


def test_no_symbol_is_defined_twice(dropin_built):
    objs = os.path.join(ORACLE_DIR, "_ref", "dropin_obj")
    theirs = set()
    for name in ("render.o", "info.o", "color.o", "timer.o"):
        theirs |= _defined(os.path.join(objs, name), dynamic=False)
    ours = _defined(LIB, dynamic=True)
    assert any(s.startswith("Color::") for s in theirs) and any(s.startswith("Info::measure") for s in theirs)
    clash = sorted(theirs & ours)
    assert not clash, clash


def test_without_a_gpu_it_ends_like_the_reference(dropin_built, tmp_path):
    import opencl_raytracer_amd as rt_mod

    if rt_mod.device_count() > 0:
        pytest.skip("a GPU is visible")
    r = subprocess.run([dropin_built, "-w", "32", "-h", "32", mesh_file("blob"), str(tmp_path / "o.pgm")],
                       capture_output=True, text=True)
    assert r.returncode != 0
    assert "Building BVH" in r.stdout           # the reference's own phase line, from its own Info::measure
    assert "No device found" in r.stderr        # reference src/opencl_host.cc:30-31


@pytest.mark.gpu
@pytest.mark.parametrize("binary", [DROPIN, DROPIN_RING], ids=["HipHost", "HipHostRing"])
def test_reference_main_renders_the_golden_pgm_on_the_hip_host(golden, tmp_path, binary):
    DROPIN = binary  # noqa: N806 (the reference's own main(), on the plain host and on the frame ring)
    if not os.path.exists(DROPIN):
        pytest.skip("oracle/_ref/ref_render_dropin* not built (needs the reference tree at build time)")
    # (no `-r` / `-m` here: the reference's own option parser returns a reference to a temporary for enum options,
    # include/args.h:233 -- g++ warns about it -- and its main() then crashes at -O2 before any of our code runs)
    for name, extra in (("bunny_256_s1_a3", []), ("bunny_600_defaults", []), ("blob_128x96_s4_a3", [])):
        c = golden["renders"][name]
        out = tmp_path / (name + ".pgm")
        cmd = [DROPIN, "-w", str(c["width"]), "-h", str(c["height"]), "-s", str(c["ss"]), "-a", str(c["ao"]),
               "-d", str(c["aod"]), "-f", str(c["focal"])] + extra + [mesh_file(c["mesh"]), str(out)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        for phase in ("Building BVH", "Loading OpenCL kernel", "Rendering image", "Loading memory", "Resizing image on host"):
            assert phase in r.stdout, phase  # reference src/render.cc:77-120, printed by its own code
        assert hashlib.md5(out.read_bytes()).hexdigest() == c["pgm_md5"], name
