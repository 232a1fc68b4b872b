"""One SHA-256 over the outputs of amp_rope_attention / amp_rope_attention_causal at fixed cases (head dimensions 64 and 96, T in
{2, 65, 129, 600}, no mask and a mask with holes, q | k | v strided views of one tensor): two builds of the library whose digests are equal
run the same attention kernels at those head dimensions.  ``AMP_LIB_PATH=<other build> python tools/attention_digest.py`` for the A/B."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from amphion_amd.modules import hip_ops  # noqa: E402


def main():
    h = hashlib.sha256()
    B, H = 2, 2
    for dk in (64, 96):
        for T in (2, 65, 129, 600):
            g = torch.Generator().manual_seed(1000 * dk + T)
            C = H * dk
            qkv = torch.randn(B, 3 * C, T, generator=g).cuda()
            mask = torch.rand(B, T, generator=g) > 0.4
            mask[:, 0] = True
            cos, sin = hip_ops.rope_tables(T, dk, qkv.device)
            for m in (None, mask.cuda()):
                for causal in (False, True):
                    out = hip_ops.rope_attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], H, cos, sin, m, causal=causal)
                    h.update(out.cpu().numpy().tobytes())
    print("attention digest", h.hexdigest())


if __name__ == "__main__":
    main()
