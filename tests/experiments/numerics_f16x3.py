"""CPU emulation of the split-f16 (3 x f16 MFMA, f32 accumulate) operand rounding, end to end through
HiFi-GAN V1, against an fp64 run of the oracle.  Design-time experiment for conv_f16x3.hip.
The emulation itself lives in tests/f16x3_emulation.py (shared with tests/test_recipe_numerics.py)."""
import sys, os
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import torch, torch.nn.functional as F
import f16x3_emulation as emu
from oracle import synth, vocoder_oracle as vo

mode = {"on": False, "terms": 3}
_c1, _ct = F.conv1d, F.conv_transpose1d

def conv1d(x, w, b=None, **kw):
    if not mode["on"]:
        return _c1(x, w, b, **kw)
    return emu.conv(x, w, b, terms=mode["terms"], **kw)

def convt(x, w, b=None, **kw):
    if not mode["on"]:
        return _ct(x, w, b, **kw)
    return emu.conv(x, w, b, transposed=True, terms=mode["terms"], **kw)

F.conv1d, F.conv_transpose1d = conv1d, convt
hp = vo.hifigan_v1_hp()
sd = synth.synth_state_dict(synth.hifigan_param_shapes(80, hp), 1234)
mel = synth.synth_mel(2, 80, 48, seed=3)
with torch.no_grad():
    ref64 = vo.hifigan_forward(sd, hp, mel, dtype=torch.float64)
    ref32 = vo.hifigan_forward(sd, hp, mel)
    mode["on"] = True
    y3 = vo.hifigan_forward(sd, hp, mel)
    mode["terms"] = "no_wlo_xhi"   # weights rounded to f16 (11 bits), activations split: 2 MFMAs per term
    yw = vo.hifigan_forward(sd, hp, mel)
    mode["terms"] = "no_wh_xlo"    # activations rounded to f16, weights split: 2 MFMAs per term
    yx = vo.hifigan_forward(sd, hp, mel)
print("out absmax", ref64.abs().max().item())
print("fp32 oracle vs fp64:", (ref32.double() - ref64).abs().max().item())
print("f16x3       vs fp64:", (y3.double() - ref64).abs().max().item())
print("f16x2 (W 11b) vs fp64:", (yw.double() - ref64).abs().max().item())
print("f16x2 (X 11b) vs fp64:", (yx.double() - ref64).abs().max().item())
