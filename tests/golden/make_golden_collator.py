"""Golden output of the reference's VocoderCollator (models/vocoders/vocoder_dataset.py:229-264) on one ragged batch, for
tests/test_reference_cli_dropin.py::test_collator_matches_reference.  CPU:

    python tests/golden/make_golden_collator.py <Amphion checkout>

writes tests/golden/golden_collator.npz: the batch's inputs (in_<i>_<key>), the collated tensors (out_<key>) and their order (keys).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LENS = [5, 3, 9, 1]


def make_batch():
    rng = np.random.default_rng(0)
    return [{"target_len": n, "mel": rng.standard_normal((4, n)).astype(np.float32),
             "frame_pitch": rng.standard_normal(n).astype(np.float32),
             "audio": rng.standard_normal(n * 8).astype(np.float32)} for n in LENS]


def main(ref_dir):
    sys.path[:0] = [os.path.join(ROOT, "tests", "shims"), ref_dir]
    from models.vocoders.vocoder_dataset import VocoderCollator

    batch = make_batch()
    out = VocoderCollator(None)(batch)
    arrays = {"keys": np.array(list(out)), "lens": np.array(LENS)}
    for i, item in enumerate(batch):
        for k in ("mel", "frame_pitch", "audio"):
            arrays[f"in_{i}_{k}"] = item[k]
    for k, v in out.items():
        arrays[f"out_{k}"] = v.numpy()
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "golden_collator.npz"), **arrays)
    print({k: (v.dtype, v.shape) for k, v in arrays.items()})


if __name__ == "__main__":
    main(sys.argv[1])
