"""CPU-only: the slot rule of the persistent tracking loops' fold (csrc/icp_fold_slots.h: icp_fold_batch_slots) and the publisher counts that feed it
(icp_level_geometry) run in a stand-alone program with a main of its own (tests/icp_fold_slots_main.cpp), built with AddressSanitizer + UBSan:
nothing of it is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fold_slot_rule_under_sanitizers(tmp_path):
    """n_wg = 1 .. 1024 publishers at 8 and 16 parts: the ladder of compiled slot counts covers every real slot, every publisher is added exactly once in
    ascending order per part, no batch polls fewer slots than it has publishers for -- and the level geometry of the images the GPU test tracks"""
    exe = str(tmp_path / "icp_fold_slots_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "hybkinectfu_amd", "csrc"), os.path.join(ROOT, "tests", "icp_fold_slots_main.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0 and "icp fold slots ok" in out.stdout, out.stdout
