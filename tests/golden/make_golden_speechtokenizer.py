"""Writes tests/golden/golden_speechtokenizer.npz and keys_speechtokenizer.json from the REAL reference classes
(models/codec/speechtokenizer/model.py) on the CPU:

    python tests/golden/make_golden_speechtokenizer.py /path/to/Amphion

The reference imports einops.  The npz holds inputs, outputs and seeds only: the weights regenerate from the seed
(tests/speechtokenizer_ref.py: synth_state_dict)."""
import json
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import speechtokenizer_ref as R  # noqa: E402

SEED = 31
SAMPLES = (1, 47, 48, 49, 480)


def main(root):
    sys.path.insert(0, root)
    warnings.simplefilter("ignore")
    from models.codec.speechtokenizer.model import SpeechTokenizer

    hp = R.small_hp()
    torch.manual_seed(0)
    model = SpeechTokenizer(hp)
    with open(os.path.join(HERE, "keys_speechtokenizer.json"), "w") as f:
        json.dump(list(model.state_dict()), f, indent=0)
    model.load_state_dict(R.synth_state_dict(hp, SEED))
    model.eval()
    out = dict(seed=np.int64(SEED))
    with torch.no_grad():
        for n in SAMPLES:
            x = R.synth_wave(2, n, 100 + n)
            z = model.encoder(x)
            codes = model.encode(x)
            o, commit, feat = model(x)
            out[f"x_{n}"] = x.numpy()
            out[f"z_{n}"] = z.numpy()
            out[f"codes_{n}"] = codes.numpy().astype(np.int16)
            out[f"dec_{n}"] = model.decode(codes).numpy()
            out[f"fwd_o_{n}"] = o.numpy()
            out[f"fwd_feat_{n}"] = feat.numpy()
            out[f"fwd_commit_{n}"] = commit.numpy()
        x = torch.from_numpy(out["x_480"])
        out["codes_st1_480"] = model.encode(x, st=1).numpy().astype(np.int16)
        out["codes_nq2_480"] = model.encode(x, n_q=2).numpy().astype(np.int16)
        out["dec_st1_480"] = model.decode(torch.from_numpy(out["codes_st1_480"]).long(), st=1).numpy()
    path = os.path.join(HERE, "golden_speechtokenizer.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
