"""Child process of test_gpu_slab_color.py: the full-size C4 colour geometry (1024^3 @ 6 m, eight LOCAL members beside the whole colour volume, ~26 GB)
in a process of its own, so that the test can give it a time limit.  Exit status 0 and "group colour c4 ok" on success."""
import torch

torch.zeros(1, device="cuda:0")          # (torch's HIP runtime first, as everywhere in the suite)

import test_gpu_slab_color as T          # noqa: E402

if __name__ == "__main__":
    T.c4_eight_colour_members()
    print("group colour c4 ok")
