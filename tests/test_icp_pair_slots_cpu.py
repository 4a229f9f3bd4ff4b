"""CPU-only: the pair rules of the persistent tracking loops' exchange (csrc/icp_fold_slots.h: which 16-byte unit carries which two sums, which lane stores
it, which lane of the fold polls it) run in a stand-alone program with a main of its own (tests/icp_pair_slots_main.cpp), built with AddressSanitizer +
UBSan: nothing of it is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pair_rules_under_sanitizers(tmp_path):
    """n_wg = 1 .. 1024 publishers at 8 and 16 parts: every (publisher, sum) is added exactly once, in ascending order per part, the padding half of the
    last pair reaches no total, every polled unit lies in the slot array -- and every pair is stored by one lane that finds its partner in its own row"""
    exe = str(tmp_path / "icp_pair_slots_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "hybkinectfu_amd", "csrc"), os.path.join(ROOT, "tests", "icp_pair_slots_main.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0 and "icp pair slots ok" in out.stdout, out.stdout
