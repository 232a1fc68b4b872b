"""The bits of the three f16x3 two-GEMM / pointwise kernels that share csrc/wholek_f16x3.h (pw_f16x3.hip, dw_layer_f16x3.hip,
codec_unit_f16x3.hip), pinned: SHA-256 of the raw fp32 output bytes of the op-level entry points on CPU-seeded inputs, against
tests/golden/wholek_digests.json.  The digests were recorded on an MI355X from a build of the commit the JSON names -- the parent of the
change that moved these kernels onto the shared header -- by calling `digest(case)` below for every case: they are what the kernels
computed BEFORE, not what the code under test gives.  A refactor of the shared text that changes a summation order, a split or a store
shows here as a different digest; the fp64 tests of the three kernels (test_gpu_vocos.py, test_gpu_diffwave.py, test_gpu_codec.py)
say whether the new bits are still right.

The cases are the smallest that reach every template form and edge of the shared code: pw small tile ragged in K, M and N / small tile
exact / the 128 x 128 tile (B * ceil(T / 128) * ceil(cout / 128) = 512 workgroups, pw_launch's threshold), each epilogue, and a strided
input; the DiffWave layer at NPW = 1 and 2, with every side tap outside [0, L), with K not a multiple of 16, with and without skip_in;
the codec unit at NPW = 1, 2, 3, T = 1, and a halo wider than the second tile."""
import hashlib
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import diffwave_ref as D  # noqa: E402
from test_gpu_codec import make_unit, unit_state_dict  # noqa: E402
from test_gpu_diffwave import layer_inputs, make_model, op_layer  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DIGESTS = os.path.join(ROOT, "tests", "golden", "wholek_digests.json")

PW = [(100, 300, 2, 65), (384, 1152, 1, 64), (384, 512, 64, 129)]                     # (cin, cout, B, T)
DW = [(32, 80, 1, 65, 1), (64, 80, 2, 63, 512), (128, 100, 1, 200, 2)]               # (C, n_mel, B, L, d)
CU = [(32, 1, 2, 1), (96, 9, 2, 65), (192, 3, 1, 200)]                               # (C, d, B, T)
EPI = ("bias", "gelu", "scale_res")


def case_ids():
    ids = [f"pw-{cin}x{cout}-B{B}-T{T}-{e}" for cin, cout, B, T in PW for e in EPI]
    ids += [f"pw-{PW[0][0]}x{PW[0][1]}-B{PW[0][2]}-T{PW[0][3]}-{e}-strided" for e in EPI]
    ids += [f"dw-C{C}-mel{M}-B{B}-L{L}-d{d}-{s}" for C, M, B, L, d in DW for s in ("skip", "noskip")]
    ids += [f"cu-C{C}-d{d}-B{B}-T{T}" for C, d, B, T in CU]
    return ids


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        assert t.dtype == torch.float32
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def _pw(cin, cout, B, T, epi, strided):
    from amphion_amd.models.codec.amphion_codec.vocos import _PwHandle, pw_forward

    g = torch.Generator().manual_seed(1000 + cin + cout + B + T)
    lin = torch.nn.Linear(cin, cout)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(cout, cin, generator=g) / cin ** 0.5)
        lin.bias.copy_(torch.randn(cout, generator=g) * 0.1)
    x = torch.randn(B, cin, T, generator=g).to(DEV)
    gamma = (torch.randn(cout, generator=g) * 0.05).to(DEV)
    y = torch.randn(B, cout, T, generator=g).to(DEV)          # the residual, updated in place (SCALE_RES); overwritten otherwise
    stride = 0
    if strided:
        wide = torch.full((B, cin + 13, T), 3e3, device=DEV)
        wide[:, 5:5 + cin] = x
        x, stride = wide[:, 5:5 + cin], (cin + 13) * T
    pw_forward(_PwHandle(), lin, x, epi, y, gamma=gamma if epi == 2 else None, res=y if epi == 2 else None, x_batch_stride=stride)
    return _sha(y)


_NETS = {}


def _dw(C, n_mel, B, L, d, skip):
    if (C, n_mel) not in _NETS:
        hp = dict(C=C, N=10, cycle=10, n_mel=n_mel, u=(16, 16))
        _NETS[(C, n_mel)] = make_model(hp, D.synth_state_dict(C, 10, n_mel, (16, 16), 2000 + C + n_mel))
    i = d.bit_length() - 1                                      # layer i of a cycle of 10 has dilation 2^i
    x, cond, dc, skip_in = layer_inputs(C, n_mel, B, L, 3000 + C + L + d, per_item=True)
    xo, so = op_layer(_NETS[(C, n_mel)], i, x.to(DEV), cond.to(DEV), dc.to(DEV), skip_in.to(DEV) if skip else None)
    return _sha(xo, so)


def _cu(C, d, B, T):
    from amphion_amd import _lib

    import codec_ref

    _lib.check(_lib.lib().amp_set_codec_unit_fusion(1))         # wherever the kernel is built: the default policy stops at C = 96
    try:
        u = make_unit(C, d, unit_state_dict(C, 4000 + C + d))
        assert u.fused(torch.device(DEV))
    finally:
        _lib.check(_lib.lib().amp_set_codec_unit_fusion(-1))
    return _sha(u(codec_ref.synth_latent(B, C, T, 5000 + C + d + T).to(DEV)))


def digest(case):
    """the SHA-256 of one case's output bytes, in f16x3 precision, with the op-level range flag clean"""
    from amphion_amd import _lib

    _lib.set_precision("f16x3")
    kind, *rest = case.split("-")
    if kind == "pw":
        cin, cout = (int(v) for v in rest[0].split("x"))
        out = _pw(cin, cout, int(rest[1][1:]), int(rest[2][1:]), EPI.index(rest[3]), strided=len(rest) == 5)
    elif kind == "dw":
        out = _dw(int(rest[0][1:]), int(rest[1][3:]), int(rest[2][1:]), int(rest[3][1:]), int(rest[4][1:]), rest[5] == "skip")
    else:
        out = _cu(int(rest[0][1:]), int(rest[1][1:]), int(rest[2][1:]), int(rest[3][1:]))
    _lib.range_check(DEV)
    return out


@pytest.fixture(scope="module")
def recorded():
    with open(DIGESTS) as f:
        doc = json.load(f)
    assert sorted(doc["digests"]) == sorted(case_ids()), "tests/golden/wholek_digests.json does not list this module's cases"
    return doc["digests"]


@pytest.mark.parametrize("case", case_ids())
def test_bits_are_the_recorded_ones(recorded, case):
    assert digest(case) == recorded[case], case

