"""The bits of the T = 1 Linear (csrc/pw_vec.hip: amp_pw_forward_vec and amp_pw_forward_vec_ln), pinned: SHA-256 of the raw fp32 output
bytes of hip_ops.pw_forward_vec / pw_forward_vec_ln on CPU-seeded inputs, against tests/golden/pw_vec_digests.json.  The digests were recorded
on an MI355X from a build of the commit the JSON names -- the parent of the change that put the two kernels on one body, when
pw_vec_kernel (llama_ar.hip) and pw_vec_ln_kernel (valle.hip) were two texts -- by calling `digest(case)` below for every case: they are what
the kernels computed BEFORE, not what the code under test gives.  A change of the shared text that moves a K split, the order of a sum, the
statistics or the workspace layout shows here as a different digest; the fp64 tests (test_gpu_ar.py, test_gpu_valle.py) say whether new bits
are still right.

The shapes are the smallest that reach every form and edge of the body, each under a handle created in "f16x3" (16 channels a unit) and one
created in "f32" (8 channels a unit).  The plans, as the recording run printed them (units; K slices x units per slice; workgroups):

    (cin, cout)     f16x3                                   f32
    (72, 40)        8 units, 2 x 4, grid 2 x 2              9 units, 2 slices of 5 / 4, grid 2 x 2
    (1024, 1664)    64 units, 5 slices of 13/13/13/13/12,   128 units, 5 slices of 26/26/26/26/24,
                    grid 52 x 5                             grid 52 x 5
    (4096, 2752)    256 units, 4 x 64, grid 86 x 4          512 units, 4 x 128, grid 86 x 4

(72, 40): cin no multiple of a unit, cout no multiple of 32, fewer channels than threads.  (1024, 1664): a ragged last slice and waves with
unequal unit counts.  (4096, 2752): the staged slice is exactly the 1024 channels the host promises the kernel (`want` = 3 < `fit` = 4), the
LayerNorm form's cin limit, and channels beyond the four a thread keeps in registers between the two statistics passes.  B = 1, 2, 3, 8 are
the item counts NB = 1, 2, 4 (one slot empty) and 8.  Every shape runs amp_pw_forward_vec with the bias and the scale-residual epilogue,
amp_pw_forward_vec_ln with LayerNorm and bias / ReLU / residual, and amp_pw_forward_vec_ln with ln_gamma = NULL and ReLU; (72, 40) runs
them again on a row block of a wider tensor, read in place."""
import ctypes
import hashlib
import json
import math
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DIGESTS = os.path.join(ROOT, "tests", "golden", "pw_vec_digests.json")

PRECISIONS = ("f16x3", "f32")
SHAPES = [(72, 40), (1024, 1664), (4096, 2752)]                                      # (cin, cout)
BATCHES = (1, 2, 3, 8)
FORMS = ("vec_bias", "vec_scale_res", "ln_bias", "ln_relu", "ln_res", "nonorm_relu")


def case_ids():
    ids = [f"{p}-{cin}x{cout}-B{B}-{f}" for p in PRECISIONS for cin, cout in SHAPES for B in BATCHES for f in FORMS]
    ids += [f"{p}-{SHAPES[0][0]}x{SHAPES[0][1]}-B{B}-{f}-strided" for p in PRECISIONS for B in BATCHES for f in FORMS]
    return ids


_handles = {}


def handle(cin, cout, precision):
    """the amp_pw handle of a seeded Linear(cin, cout), created under ``precision`` (a handle keeps the arithmetic it was created with)"""
    from amphion_amd import _lib

    key = (cin, cout, precision)
    if key not in _handles:
        g = torch.Generator().manual_seed(7000 + cin + cout)
        w = (torch.randn(cout, cin, generator=g) / math.sqrt(cin)).contiguous()
        b = (torch.randn(cout, generator=g) * 0.1).contiguous()
        h = ctypes.c_void_p()
        before = _lib.get_precision()
        _lib.set_precision(precision)
        try:
            with torch.cuda.device(DEV):
                _lib.check(_lib.lib().amp_pw_create(cin, cout, _lib.ptr(w), _lib.ptr(b), ctypes.byref(h)))
        finally:
            _lib.set_precision(before)
        _handles[key] = h
    return _handles[key]


def free_handles():
    from amphion_amd import _lib

    torch.cuda.synchronize()
    while _handles:
        _lib.lib().amp_pw_destroy(_handles.popitem()[1])


def digest(case):
    """the SHA-256 of one case's output bytes"""
    from amphion_amd.modules import hip_ops

    precision, shape, nb, form, *rest = case.split("-")
    cin, cout = (int(v) for v in shape.split("x"))
    B = int(nb[1:])
    h = handle(cin, cout, precision)
    g = torch.Generator().manual_seed(8000 + cin + cout + B)
    x = (1.5 * torch.randn(B, cin, 1, generator=g) + 0.3).to(DEV)
    lg, lb = (1.0 + 0.2 * torch.randn(cin, generator=g)).to(DEV), (0.2 * torch.randn(cin, generator=g)).to(DEV)
    gamma = (1.0 + 0.5 * torch.randn(cout, generator=g)).to(DEV)
    res = torch.randn(B, cout, 1, generator=g).to(DEV)
    if rest:                                                    # a row block of a wider tensor, read in place through its batch stride
        wide = torch.full((B, cin + 13, 1), 3e3, device=DEV)
        wide[:, 5:5 + cin] = x
        x = wide[:, 5:5 + cin]
    if form == "vec_bias":
        y = hip_ops.pw_forward_vec(h, cout, x)
    elif form == "vec_scale_res":
        y = hip_ops.pw_forward_vec(h, cout, x, gamma=gamma, res=res)
    elif form == "ln_bias":
        y = hip_ops.pw_forward_vec_ln(h, cout, x, lg, lb, 1e-5)
    elif form == "ln_relu":
        y = hip_ops.pw_forward_vec_ln(h, cout, x, lg, lb, 1e-5, relu=True)
    elif form == "ln_res":
        y = hip_ops.pw_forward_vec_ln(h, cout, x, lg, lb, 1e-5, gamma=gamma, res=res)
    else:
        assert form == "nonorm_relu", form
        y = hip_ops.pw_forward_vec_ln(h, cout, x, relu=True)
    assert y.dtype == torch.float32 and tuple(y.shape) == (B, cout, 1)
    return hashlib.sha256(y.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


@pytest.fixture(scope="module")
def recorded():
    with open(DIGESTS) as f:
        doc = json.load(f)
    assert sorted(doc["digests"]) == sorted(case_ids()), "tests/golden/pw_vec_digests.json does not list this module's cases"
    yield doc["digests"]
    free_handles()                                              # six handles, two of them 4096 x 2752


@pytest.mark.parametrize("case", case_ids())
def test_bits_are_the_recorded_ones(recorded, case):
    assert digest(case) == recorded[case], case
