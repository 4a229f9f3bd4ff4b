"""CPU-only: what an erase decides from coordinates alone -- the class of a brick against a box and the voxel test (csrc/erase_box.h), the clamp of any
int32 box to the key range, and a box in metres as a box of voxels (host/erase_box_voxels.hpp) -- in a stand-alone program with a main of its own
(tests/map_erase_main.cpp), built with AddressSanitizer + UBSan and run as a program: nothing of it is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_brick_class_clamp_and_metres_under_sanitizers(tmp_path):
    exe = str(tmp_path / "map_erase_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "hybkinectfu_amd", "host"), "-I", os.path.join(ROOT, "hybkinectfu_amd", "csrc"),
                           os.path.join(ROOT, "tests", "map_erase_main.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0 and out.stdout.splitlines()[-1] == "map erase ok", out.stdout[-3000:]
