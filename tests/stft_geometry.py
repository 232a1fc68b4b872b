"""Tables, fp64 references and fp32 restatements for the inverse STFT (amp_istft_forward / amp_istft_same / amp_istft_same_polar) and the mel
gradient (amp_mel_backward, dense and ragged) over the geometry include/amphion_hip.h documents.  No GPU import: tests/test_stft_geometry_ref.py
checks on the CPU what the tables reach and that the bounds catch a kernel with one slip; tests/test_gpu_stft_geometry.py runs the kernels.

Every case names the classes it is there for (`why`); `*_labels()` re-derive the classes from the numbers alone.

The references are written from the definitions (utils/stft.py:183-222, apnet.py:46-101, vocos.py:346-359, utils/mel.py:111-170), not from the
kernels:
  forward     frame = irfft(X) * window * hop / n_fft (the pseudo-inverse of the basis scaled by n_fft / hop); num = overlap-add; out =
              (n_fft / hop) * num / wss where the float32 wss handed to the library exceeds float32 tiny, (n_fft / hop) * num elsewhere;
              floor(n_fft / 2) cropped per side, hop (F - 1) + (n_fft & 1) samples.  X = mag e^{i phase}
  same        frame = irfft(X) * window; out = overlap-add / envelope; (win - hop) / 2 cropped per side, F hop samples.  X = re + i im
  same_polar  the same with X = min(exp(m), clip) (cos p, sin p)
The imaginary parts of bin 0 and of the Nyquist bin are ignored; an odd n_fft has no Nyquist bin.
  gradient    autograd of the fp64 log-mel (oracle.vocoder_oracle.extract_mel_features; a restatement below for pad_mode 1, the linear mel and
              other eps) on sum(g * logmel), per utterance cut to its own length.
"""
import math
import os
import sys
from types import SimpleNamespace as NS

import numpy as np
import torch
import torch.nn.functional as Fn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from fvq_geometry import DEVICE_TENSOR_CAP  # noqa: E402,F401  (1 MiB: no device tensor of the sweep is larger, for the reason written there)
from oracle import vocoder_oracle as vo  # noqa: E402

TINY = float(np.finfo(np.float32).tiny)
REL = 2e-5                       # the relative bound of test_stft_inverse_any_smooth_nfft and of the Vocos ISTFT test
GRAD_REL = 1e-4                  # test_mel_gradient_of_a_plain_sum
SIGN_MAX, SIGN_MEAN = 2e-3, 2e-5 # test_mel_loss_value_and_gradient
POLAR_SPLIT = 1e-5               # test_istft_same_polar_against_fp64_and_split_path: same_polar against same, times the peak
OLA_BLOCK = 256                  # threads of istft_ola_kernel / mel_grad_ola_kernel
WAVE_FRAMES = 32                 # frames per workgroup of istft_wave_kernel / mel_wave_kernel / mel1024_kernel, and of mel_grad_spec_kernel's tile
SR = 16000
AMP_OK, AMP_ERR_INVALID, AMP_ERR_UNSUPPORTED = 0, -1, -4


# ------------------------------------------------------------------------------------------------------------------------------
# what the launchers select, restated from the numbers (launch_istft_frames, launch_mel in csrc/mel.hip)
# ------------------------------------------------------------------------------------------------------------------------------
def prime_factors(n):
    out, p = [], 2
    while p * p <= n:
        while n % p == 0:
            out.append(p)
            n //= p
        p += 1
    if n > 1:
        out.append(n)
    return out


def frames_form(n_fft, aligned=True):
    """the inverse frame kernel: 'wave15' (n_fft 1920 and 8-byte aligned frames / window), 'radix2', 'mixed'"""
    if n_fft == 1920 and aligned:
        return "wave15"
    return "radix2" if n_fft & (n_fft - 1) == 0 else "mixed"


def frames_lds_bytes(n_fft, aligned=True):
    form = frames_form(n_fft, aligned)
    if form == "radix2":
        return (2 * n_fft + n_fft // 2) * 8
    if form == "mixed":
        return 3 * n_fft * 8
    return None                                   # the wave kernel's request does not depend on the case


def mel_forward_form(n_fft, hop, n_mel):
    """the forward kernel launch_mel takes for pad_mode 0"""
    pad = (n_fft - hop) // 2
    even = pad % 2 == 0 and hop % 2 == 0
    if n_fft == 1024 and n_mel <= 256 and even:
        return "mel1024"
    if n_fft in (2048, 1920, 512) and even and n_mel <= 256:
        return "mel_wave"
    return "mel_mixed" if n_fft & (n_fft - 1) else "mel_kernel"


def num_frames(L, n_fft, hop, pad_mode=0):
    """amp_mel_num_frames; a ragged row also needs L > pad"""
    pad = (n_fft - hop) // 2 if pad_mode == 0 else n_fft // 2
    if L + 2 * pad < n_fft:
        return 0
    return (L + 2 * pad - n_fft) // hop + 1


def row_frames(L, n_fft, hop, pad_mode=0):
    pad = (n_fft - hop) // 2 if pad_mode == 0 else n_fft // 2
    return 0 if L <= pad else num_frames(L, n_fft, hop, pad_mode)


def truncating_row_frames(L, n_fft, hop, pad_mode=0):
    """the rule the kernels had: C division rounds (L + 2 pad - n_fft) / hop towards zero"""
    pad = (n_fft - hop) // 2 if pad_mode == 0 else n_fft // 2
    return 0 if L <= pad else int((L + 2 * pad - n_fft) / hop) + 1


# ------------------------------------------------------------------------------------------------------------------------------
# inverse STFT
# ------------------------------------------------------------------------------------------------------------------------------
class Ist:
    def __init__(self, id, mode, n_fft, hop, F, *, B=2, win=None, window="hann", form=None, offset=0, stride_extra=0, clip=None,
                 overflow=False, why=()):
        self.id, self.mode, self.n_fft, self.hop, self.F, self.B = id, mode, n_fft, hop, F, B
        self.win = n_fft if win is None else win
        self.window = window
        self.form = form or {"forward": "polar", "same": "reim", "same_polar": "head"}[mode]
        self.offset, self.stride_extra, self.clip, self.overflow = offset, stride_extra, clip, overflow
        self.why = tuple(why)
        self.bins = n_fft // 2 + 1
        self.seed = 1000 * n_fft + 10 * hop + F
        if mode == "forward":
            self.crop, self.Lout, self.scale = n_fft // 2, hop * (F - 1) + (n_fft & 1), n_fft / hop
        else:
            self.crop, self.Lout, self.scale = (self.win - hop) // 2, F * hop, 1.0
        self.Lfull = n_fft + hop * (F - 1)

    def __repr__(self):
        return self.id


ISTFT = [
    # forward mode: (magnitude, phase)
    Ist("fwd_64_q_F2", "forward", 64, 16, 2, why=("radix2", "hop_quarter", "F_min", "f0_clamped", "f1_clamped", "phase_100")),
    Ist("fwd_64_hop7_F3", "forward", 64, 7, 3, why=("hop_nondividing", "hop_odd", "F_min_plus_1")),
    Ist("fwd_64_half", "forward", 64, 32, 9, why=("hop_half", "lout_256", "f0_free", "f1_free")),
    Ist("fwd_256_hop100", "forward", 256, 100, 5, why=("hop_nondividing", "lout_straddles_block")),
    Ist("fwd_256_hop85", "forward", 256, 85, 4, why=("lout_255", "hop_odd")),
    Ist("fwd_256_full", "forward", 256, 256, 3, why=("hop_full", "wss_zero_at_joint", "tiny_skip", "tiny_divide")),
    Ist("fwd_81_hop64", "forward", 81, 64, 5, why=("odd_nfft", "lout_257", "mixed")),
    Ist("fwd_81_hop20", "forward", 81, 20, 14, why=("odd_nfft", "hop_nondividing")),
    Ist("fwd_2048_q", "forward", 2048, 512, 9, why=("radix2", "hop_quarter")),
    Ist("fwd_4096_q", "forward", 4096, 1024, 6, why=("radix2", "lds_optin")),
    Ist("fwd_1920_31", "forward", 1920, 480, 31, B=1, why=("wave15", "wave_frames_31")),
    Ist("fwd_1920_32", "forward", 1920, 480, 16, why=("wave15", "wave_frames_32")),
    Ist("fwd_1920_33", "forward", 1920, 480, 11, B=3, why=("wave15", "wave_frames_33")),
    Ist("fwd_1920_65", "forward", 1920, 480, 13, B=5, why=("wave15", "wave_frames_65")),
    Ist("fwd_1920_unaligned", "forward", 1920, 480, 16, offset=1, why=("mixed", "frames_unaligned")),
    Ist("fwd_400_q", "forward", 400, 100, 7, why=("mixed", "hop_quarter")),
    Ist("fwd_400_full_win300", "forward", 400, 400, 3, win=300, why=("hop_full", "win_short", "tiny_skip", "tiny_divide")),
    Ist("fwd_646_win600", "forward", 646, 323, 4, win=600, why=("mixed", "hop_half", "win_short")),
    Ist("fwd_1000_half_win400", "forward", 1000, 500, 4, win=400, why=("win_short", "tiny_skip", "tiny_divide")),
    Ist("fwd_4000_q", "forward", 4000, 1000, 4, why=("mixed", "lds_optin")),
    Ist("fwd_1001_hop143", "forward", 1001, 143, 9, why=("odd_nfft", "hop_odd", "f0_free")),
    Ist("fwd_4095_third", "forward", 4095, 1365, 4, why=("odd_nfft", "lds_optin")),
    Ist("fwd_68_q", "forward", 68, 17, 6, why=("generic_pass",)),
    Ist("fwd_67_prime", "forward", 67, 16, 5, why=("prime", "generic_pass", "odd_nfft")),
    Ist("fwd_1021_prime", "forward", 1021, 255, 8, why=("prime", "generic_pass")),
    # same mode: (re, im)
    Ist("same_64_F1", "same", 64, 16, 1, why=("F_min", "radix2", "reim")),
    Ist("same_256_F2", "same", 256, 128, 2, why=("F_min_plus_1", "lout_256", "hop_half")),
    Ist("same_256_full_hamming", "same", 256, 256, 2, window="hamming", why=("hop_full",)),
    Ist("same_1001_hop85", "same", 1001, 85, 3, why=("lout_255", "odd_nfft", "hop_nondividing", "hop_odd")),
    Ist("same_1001_hop257_F1", "same", 1001, 257, 1, why=("lout_257", "F_min")),
    Ist("same_1920", "same", 1920, 480, 16, why=("wave15", "wave_frames_32")),
    Ist("same_1920_unaligned", "same", 1920, 480, 16, offset=1, why=("mixed", "frames_unaligned")),
    Ist("same_4000", "same", 4000, 1000, 3, why=("mixed", "lds_optin")),
    Ist("same_4095", "same", 4095, 1365, 3, why=("odd_nfft", "lds_optin")),
    Ist("same_67", "same", 67, 17, 3, why=("prime",)),
    Ist("same_68_hop18", "same", 68, 18, 4, why=("generic_pass", "hop_nondividing")),
    Ist("same_646", "same", 646, 160, 5, why=("mixed",)),
    Ist("same_1021", "same", 1021, 255, 8, why=("prime",)),
    # same_polar: the head slab
    Ist("polar_256", "same_polar", 256, 64, 5, clip=1e9, why=("radix2", "head")),
    Ist("polar_400_clipped", "same_polar", 400, 100, 6, stride_extra=7, clip=3.0, overflow=True,
        why=("mixed", "head_strided", "clipped", "exp_overflow")),
    Ist("polar_1920", "same_polar", 1920, 480, 8, stride_extra=1920 + 5, clip=1e9, why=("wave15", "head_strided")),
    Ist("polar_1920_65", "same_polar", 1920, 480, 13, B=5, clip=20.0, why=("wave15", "wave_frames_65", "clipped")),
    Ist("polar_2048", "same_polar", 2048, 512, 5, clip=1e9, why=("radix2", "head")),
    Ist("polar_4096", "same_polar", 4096, 1024, 4, clip=1e9, why=("radix2", "lds_optin")),
    Ist("polar_81_F1", "same_polar", 81, 27, 1, clip=1e9, why=("odd_nfft", "F_min")),
]
ISTFT_REQUIRED = ("radix2", "mixed", "wave15", "lds_optin", "generic_pass", "prime", "odd_nfft", "frames_unaligned",
                  "hop_quarter", "hop_half", "hop_full", "hop_nondividing", "hop_odd",
                  "fwd:F_min", "fwd:F_min_plus_1", "same:F_min", "same:F_min_plus_1", "same_polar:F_min",
                  "wave_frames_31", "wave_frames_32", "wave_frames_33", "wave_frames_65", "lout_255", "lout_256", "lout_257",
                  "f0_clamped", "f0_free", "f1_clamped", "f1_free", "tiny_skip", "tiny_divide", "wss_zero_at_joint", "win_short",
                  "polar", "phase_100", "reim", "head", "head_strided", "clipped", "exp_overflow",
                  "lds:81920", "lds:96000", "lds:98280")
POLAR_SPLIT_CASES = ("polar_256", "polar_400_clipped", "polar_1920")          # one per kernel form


def ist_by_id(name):
    return next(c for c in ISTFT if c.id == name)


def ist_window32(c):
    """the float32 window handed to the library: periodic, centre-padded to n_fft"""
    n = np.arange(c.win, dtype=np.float64)
    a = (0.5, 0.5) if c.window == "hann" else (0.54, 0.46)
    w = a[0] - a[1] * np.cos(2.0 * np.pi * n / c.win)
    lp = (c.n_fft - c.win) // 2
    return np.pad(w, (lp, c.n_fft - c.win - lp)).astype(np.float32)


def ist_den32(c):
    """the float32 window-sum-square (forward) / envelope (same) handed to the library: [n_fft + hop (F - 1)]"""
    w2 = ist_window32(c).astype(np.float64) ** 2
    x = np.zeros(c.Lfull)
    for f in range(c.F):
        x[f * c.hop:f * c.hop + c.n_fft] += w2
    return x.astype(np.float32)


def ist_inputs(c):
    """float32 inputs as the entry point takes them.  The spectra are those of random frames in [-1, 1], so irfft gives O(1) samples; the
    imaginary parts of bin 0 and of the Nyquist bin are NOT zero."""
    g = torch.Generator().manual_seed(c.seed)
    x = torch.rand(c.B, c.F, c.n_fft, generator=g, dtype=torch.float64) * 2 - 1
    X = torch.fft.rfft(x, dim=-1).transpose(1, 2).contiguous()                      # [B, bins, F]
    re, im = X.real.clone(), X.imag.clone()
    edge = [0] + ([c.n_fft // 2] if c.n_fft % 2 == 0 else [])
    im[:, edge] = (torch.rand(c.B, len(edge), c.F, generator=g, dtype=torch.float64) * 2 - 1) * re[:, edge].abs().clamp(min=1.0)
    if c.form == "reim":
        return {"re": re.float(), "im": im.float()}
    mag = torch.sqrt(re * re + im * im)
    turns = torch.randint(-15, 16, mag.shape, generator=g).double()
    phase = torch.atan2(im, re) + 2 * math.pi * turns
    if c.form == "polar":
        return {"mag": mag.float(), "phase": phase.float()}
    logm = torch.log(mag.clamp(min=1e-30))
    if c.overflow:
        logm[c.B - 1, c.bins // 3, c.F // 2] = 100.0                                   # expf -> inf in fp32; clips to mag_clip
    rows = 2 * c.bins
    stride = rows * c.F + c.stride_extra
    head = torch.full((c.B, stride), float("nan"), dtype=torch.float32)              # the gap between the items is never read
    head[:, :rows * c.F] = torch.cat([logm, phase], 1).float().reshape(c.B, -1)
    return {"head": head, "stride": stride, "clip": float(c.clip)}


def ist_spectrum(c, inp, dtype=torch.float64):
    """(re, im) [B, bins, F] in `dtype` from the float32 inputs"""
    if c.form == "reim":
        return inp["re"].to(dtype), inp["im"].to(dtype)
    if c.form == "polar":
        m, p = inp["mag"].to(dtype), inp["phase"].to(dtype)
    else:
        h = inp["head"][:, :2 * c.bins * c.F].reshape(c.B, 2 * c.bins, c.F).to(dtype)
        m = torch.clamp(torch.exp(h[:, :c.bins]), max=inp["clip"])
        p = h[:, c.bins:]
    return m * torch.cos(p), m * torch.sin(p)


def ist_reference(c, inp):
    """fp64: {'out' [B, Lout], 'num' [B, Lout] the overlap-add, 'den' [Lout] what the kernel divides by (1 where it does not), 'c'}"""
    re, im = ist_spectrum(c, inp)
    im = im.clone()
    im[:, 0] = 0.0
    if c.n_fft % 2 == 0:
        im[:, c.n_fft // 2] = 0.0
    x = torch.fft.irfft(torch.complex(re, im), n=c.n_fft, dim=1)                      # [B, n_fft, F]
    w = torch.from_numpy(ist_window32(c)).double()
    fr = x * w[None, :, None] / c.scale
    full = torch.zeros(c.B, c.Lfull, dtype=torch.float64)
    for f in range(c.F):
        full[:, f * c.hop:f * c.hop + c.n_fft] += fr[:, :, f]
    num = full[:, c.crop:c.crop + c.Lout]
    d32 = torch.from_numpy(ist_den32(c))[c.crop:c.crop + c.Lout]
    divides = d32 > TINY if c.mode == "forward" else torch.ones_like(d32, dtype=torch.bool)
    den = torch.where(divides, d32.double(), torch.ones_like(d32, dtype=torch.float64))
    return {"out": num / den * c.scale, "num": num, "den": den, "c": c.scale}


def ist_bound(ref):
    """[Lout]: |err[m]| <= 2e-5 c max(1, max |num64|) / den[m]"""
    return REL * ref["c"] * max(1.0, float(ref["num"].abs().max())) / ref["den"]


def ist_excess(ref, out):
    """largest error / bound; inf for a shape mismatch or a non-finite output"""
    out = torch.as_tensor(np.asarray(out)).double() if not isinstance(out, torch.Tensor) else out.detach().cpu().double()
    if out.shape != ref["out"].shape or not bool(torch.isfinite(out).all()):
        return math.inf
    return float(((out - ref["out"]).abs() / ist_bound(ref)[None, :]).max())


def ola_ranges(c):
    """(m, f0, f1) of istft_ola_kernel for every output sample"""
    m = np.arange(c.Lout) + c.crop
    f0 = np.where(m - c.n_fft + 1 <= 0, 0, (m - c.n_fft + c.hop) // c.hop)
    f1u = m // c.hop
    return m, f0, np.minimum(f1u, c.F - 1), f1u


def ist_labels(c, inp=None):
    inp = inp or ist_inputs(c)
    aligned = c.offset == 0
    form = frames_form(c.n_fft, aligned)
    out = {form, c.form}
    lds = frames_lds_bytes(c.n_fft, aligned)
    if lds and lds > 64 * 1024:
        out |= {"lds_optin", f"lds:{lds}"}
    pf = prime_factors(c.n_fft)
    if form == "mixed" and max(pf) > 13:
        out.add("generic_pass")
    if len(pf) == 1:
        out.add("prime")
    if c.n_fft % 2:
        out.add("odd_nfft")
    if not aligned and c.n_fft == 1920:
        out.add("frames_unaligned")
    if 4 * c.hop == c.n_fft:
        out.add("hop_quarter")
    if 2 * c.hop == c.n_fft:
        out.add("hop_half")
    if c.hop == c.n_fft:
        out.add("hop_full")
    if c.n_fft % c.hop:
        out.add("hop_nondividing")
    if c.hop % 2:
        out.add("hop_odd")
    fmin = 2 if c.mode == "forward" else 1
    if c.F == fmin:
        out.add("F_min")
    if c.F == fmin + 1:
        out.add("F_min_plus_1")
    if form == "wave15":
        out.add(f"wave_frames_{c.B * c.F}")
    if c.Lout in (255, 256, 257):
        out.add(f"lout_{c.Lout}")
    if c.Lout > OLA_BLOCK and c.Lout % OLA_BLOCK:
        out.add("lout_straddles_block")
    m, f0, f1, f1u = ola_ranges(c)
    out.add("f0_clamped" if (m - c.n_fft + 1 <= 0).any() else "")
    out.add("f0_free" if (m - c.n_fft + 1 > 0).any() else "")
    out.add("f1_clamped" if (f1u > c.F - 1).any() else "")
    out.add("f1_free" if (f1u <= c.F - 1).any() else "")
    if c.win < c.n_fft:
        out.add("win_short")
    if c.mode == "forward":
        d = ist_den32(c)[c.crop:c.crop + c.Lout]
        if (d <= TINY).any():
            out.add("tiny_skip")
        if (d > TINY).any():
            out.add("tiny_divide")
        joints = [f * c.hop - c.crop for f in range(1, c.F) if 0 <= f * c.hop - c.crop < c.Lout]
        if c.hop == c.n_fft and joints and all(d[j] == 0 for j in joints):
            out.add("wss_zero_at_joint")
        if float(inp["phase"].abs().max()) >= 90:
            out.add("phase_100")
    if c.form == "head":
        if c.stride_extra:
            out.add("head_strided")
        h = inp["head"][:, :2 * c.bins * c.F].reshape(c.B, 2 * c.bins, c.F)[:, :c.bins]
        e32 = torch.exp(h)
        if bool(((e32 > inp["clip"]) & torch.isfinite(e32)).any()):
            out.add("clipped")
        if bool(torch.isinf(e32).any()):
            out.add("exp_overflow")
    out.discard("")
    return out


def ist_required_reached():
    have = set()
    for c in ISTFT:
        lab = ist_labels(c)
        have |= lab
        mode = {"forward": "fwd", "same": "same", "same_polar": "same_polar"}[c.mode]
        have |= {f"{mode}:{v}" for v in lab if v.startswith("F_min")}
    return have


ISTFT_MUTANTS = ("lost_partner", "nyquist_imag_kept", "odd_as_nyquist", "f0_plus_one", "f1_minus_one", "crop_plus_one", "tiny_dropped")


def _gather_ola(frames, t, fa, fz, hop):
    """sum over f in [fa, fz] of frames[f, t - f hop], float32, f ascending as the kernels add"""
    acc = np.zeros(t.shape, np.float32)
    span = int((fz - fa).max()) + 1 if t.size else 0
    for j in range(max(span, 0)):
        f = fa + j
        ok = f <= fz
        fs = np.where(ok, f, 0)
        idx = np.where(ok, t - fs * hop, 0)
        acc = acc + np.where(ok, frames[fs, idx], np.float32(0))
    return acc


def ist_model(c, inp, mutant=None):
    """float32 restatement of the kernels' arithmetic: the spectrum in float32, the Hermitian extension (the packed half-length transform for the
    wave kernel), the zeroed imaginary parts, inv_scale / n_fft, the window, istft_ola_kernel's index range, crop and tiny rule."""
    re, im = ist_spectrum(c, inp, torch.float32)
    X = (re.double().numpy() + 1j * im.double().numpy())                            # [B, bins, F]
    n, half = c.n_fft, c.n_fft // 2
    nyq = half if (n % 2 == 0 or mutant == "odd_as_nyquist") else -1
    X[:, 0] = X[:, 0].real
    if nyq >= 0 and mutant != "nyquist_imag_kept":
        X[:, nyq] = X[:, nyq].real
    if frames_form(n, c.offset == 0) == "wave15" and mutant in (None, "nyquist_imag_kept"):
        k = np.arange(half)
        Xk, Xp = X[:, :half], np.conj(X[:, half - k])
        Z = (Xk + Xp) / 2 + 1j * np.exp(2j * np.pi * k / n)[None, :, None] * (Xk - Xp) / 2
        z = np.fft.ifft(Z, axis=1)
        x = np.empty((c.B, n, c.F))
        x[:, 0::2], x[:, 1::2] = z.real, z.imag
    else:
        full = np.zeros((c.B, n, c.F), complex)
        full[:, :c.bins] = X
        last = c.bins - 1 if nyq < 0 else nyq - 1                                      # the last bin that has a partner
        for kk in range(1, last + 1):
            if kk != nyq and not (mutant == "lost_partner" and kk == last):           # (ONE partner lost: a loop that stops one bin early)
                full[:, n - kk] = np.conj(X[:, kk])
        x = np.fft.ifft(full, axis=1).real
    sc = np.float32(np.float32(1.0 / np.float32(c.scale)))
    fr = (x.astype(np.float32) * sc * ist_window32(c)[None, :, None]).astype(np.float32)
    fr = np.ascontiguousarray(fr.transpose(0, 2, 1))                                   # [B, F, n_fft]
    crop = c.crop + (1 if mutant == "crop_plus_one" and c.crop + c.Lout < c.Lfull else 0)      # (crop 0 of hop = win: nothing behind the range)
    m = np.arange(c.Lout) + crop
    f0 = np.where(m - n + 1 <= 0, 0, (m - n + c.hop) // c.hop)
    f1 = np.minimum(m // c.hop, c.F - 1)
    if mutant == "f0_plus_one":
        f0 = f0 + 1
    if mutant == "f1_minus_one":
        f1 = f1 - 1
    den = ist_den32(c)[m]
    tiny = np.float32(TINY) if c.mode == "forward" else np.float32(-1.0)
    out = np.empty((c.B, c.Lout), np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        for b in range(c.B):
            acc = _gather_ola(fr[b], m, f0, f1, c.hop)
            if mutant == "tiny_dropped":
                acc = acc / den
            else:
                acc = np.where(den > tiny, acc / np.where(den > tiny, den, np.float32(1)), acc)
            out[b] = acc * np.float32(c.scale)
    return out


def envelope_floor(c):
    """smallest envelope over the cropped range / its maximum (the `same` modes always divide)"""
    d = ist_den32(c).astype(np.float64)
    return float(d[c.crop:c.crop + c.Lout].min() / d.max())


# ------------------------------------------------------------------------------------------------------------------------------
# refusals: (id, entry point, what to change on a valid call, status)
# ------------------------------------------------------------------------------------------------------------------------------
REFUSALS = [
    ("forward_F1", "forward", dict(F=1), AMP_ERR_INVALID),
    ("forward_F0", "forward", dict(F=0), AMP_ERR_INVALID),
    ("forward_hop_above_nfft", "forward", dict(hop=257), AMP_ERR_INVALID),
    ("forward_nfft_63", "forward", dict(n_fft=63, win=63, hop=16), AMP_ERR_UNSUPPORTED),
    ("forward_nfft_4097", "forward", dict(n_fft=4097, win=4097), AMP_ERR_UNSUPPORTED),
    ("forward_null_wss", "forward", dict(null="den"), AMP_ERR_INVALID),
    ("forward_null_frames", "forward", dict(null="frames"), AMP_ERR_INVALID),
    ("same_F0", "same", dict(F=0), AMP_ERR_INVALID),
    ("same_hop_above_nfft", "same", dict(hop=258), AMP_ERR_INVALID),
    ("same_odd_win_minus_hop", "same", dict(hop=63), AMP_ERR_INVALID),
    ("same_win_not_nfft", "same", dict(win=200), AMP_ERR_UNSUPPORTED),
    ("same_nfft_4098", "same", dict(n_fft=4098, win=4098), AMP_ERR_UNSUPPORTED),
    ("same_null_im", "same", dict(null="b"), AMP_ERR_INVALID),
    ("polar_F0", "same_polar", dict(F=0), AMP_ERR_INVALID),
    ("polar_odd_win_minus_hop", "same_polar", dict(hop=65), AMP_ERR_INVALID),
    ("polar_win_not_nfft", "same_polar", dict(win=200), AMP_ERR_INVALID),
    ("polar_nfft_62", "same_polar", dict(n_fft=62, win=62, hop=16), AMP_ERR_INVALID),
    ("polar_stride_too_small", "same_polar", dict(stride=-1), AMP_ERR_INVALID),
    ("polar_clip_zero", "same_polar", dict(clip=0.0), AMP_ERR_INVALID),
    ("polar_clip_negative", "same_polar", dict(clip=-1.0), AMP_ERR_INVALID),
    ("polar_null_head", "same_polar", dict(null="a"), AMP_ERR_INVALID),
    ("polar_null_wav", "same_polar", dict(null="wav"), AMP_ERR_INVALID),
]
REFUSAL_BASE = dict(n_fft=256, win=256, hop=64, F=4, B=2)


# ------------------------------------------------------------------------------------------------------------------------------
# mel gradient
# ------------------------------------------------------------------------------------------------------------------------------
class Grad:
    def __init__(self, id, n_fft, hop, n_mel, L, *, B=2, pad_mode=0, log_clip=1e-5, mag_eps=1e-9, lens=None, g="smooth", zero_row=None, why=()):
        self.id, self.n_fft, self.hop, self.n_mel, self.L, self.B = id, n_fft, hop, n_mel, L, B
        self.pad_mode, self.log_clip, self.mag_eps, self.g, self.zero_row = pad_mode, log_clip, mag_eps, g, zero_row
        self.lens = list(lens) if lens is not None else None
        if self.lens is not None:
            assert len(self.lens) == B and max(self.lens) == L and self.lens[0] == L
        self.why = tuple(why)
        self.bins = n_fft // 2 + 1
        self.pad = (n_fft - hop) // 2 if pad_mode == 0 else n_fft // 2
        self.F = num_frames(L, n_fft, hop, pad_mode)
        self.seed = 77 * n_fft + hop + L
        self.pp = NS(sample_rate=SR, n_fft=n_fft, win_size=n_fft, hop_size=hop, n_mel=n_mel, fmin=0, fmax=None)

    def counts(self):
        return [row_frames(n, self.n_fft, self.hop, self.pad_mode) for n in (self.lens or [self.L] * self.B)]

    def __repr__(self):
        return self.id


def _ragged_lens(n_fft, hop):
    """row 0 full, a row with pad < len < hop, a row off the hop grid, a row with len <= pad"""
    pad = (n_fft - hop) // 2
    return [5 * hop + 3, pad + 1 + (hop - pad - 1) // 2, 3 * hop + 7, pad]


GRAD = [
    Grad("g64_F31", 64, 16, 8, 511, why=("F_31", "L_255")),
    Grad("g64_F32", 64, 16, 8, 512, why=("F_32", "L_0")),
    Grad("g64_F32b", 64, 16, 8, 513, why=("F_32", "L_1")),
    Grad("g64_F33", 64, 16, 8, 528, why=("F_33",)),
    Grad("g64_taco_lin", 64, 16, 8, 496, pad_mode=1, log_clip=0.0, why=("pad_mode_1", "linear", "F_32")),
    Grad("g256_hop100", 256, 100, 13, 3300, why=("F_33", "n_mel_off_8", "hop_above_third")),
    Grad("g400_F1", 400, 160, 80, 200, why=("F_1", "hop_above_third")),
    Grad("g400_F32", 400, 160, 80, 5120, why=("F_32", "L_0")),
    Grad("g512_F1", 512, 256, 40, 256, why=("F_1", "L_0")),
    Grad("g512_F1b", 512, 256, 40, 257, why=("F_1", "L_1")),
    Grad("g512_F31", 512, 256, 40, 7936, why=("F_31",)),
    Grad("g512_zero_row", 512, 256, 40, 2048, log_clip=0.0, mag_eps=0.0, zero_row=1, why=("zero_row", "linear")),
    Grad("g1001", 1001, 501, 40, 1503, why=("odd_nfft", "hop_above_third")),
    Grad("g1001_taco", 1001, 501, 40, 2004, pad_mode=1, why=("pad_mode_1", "odd_nfft")),
    Grad("g1024_F32", 1024, 256, 80, 8192, why=("F_32",)),
    Grad("g1024_sign", 1024, 256, 80, 8448, g="sign", why=("F_33", "sign_pattern")),
    Grad("g1920_F33", 1920, 480, 100, 15840, why=("F_33", "wave15", "n_mel_off_8")),
    Grad("g1920_taco_lin", 1920, 480, 100, 4800, pad_mode=1, log_clip=-1.0, why=("pad_mode_1", "linear")),
    Grad("g2048_F31", 2048, 512, 128, 15872, why=("F_31",)),
    Grad("g68", 68, 17, 5, 561, why=("generic_pass", "n_mel_off_8")),
    Grad("g4096_F4", 4096, 1024, 128, 4096, B=1, why=("lds_optin",)),
    Grad("g4096_F33", 4096, 1024, 128, 33792, B=1, why=("lds_optin", "F_33")),
] + [
    Grad(f"g{n}_ragged", n, h, nm, _ragged_lens(n, h)[0], B=4, lens=_ragged_lens(n, h), why=("ragged", "zero_frame_short", "zero_frame_pad", "off_grid"))
    for n, h, nm in ((256, 100, 13), (400, 160, 80), (512, 256, 40), (1001, 501, 40))
]
GRAD_CONFIGS = ((64, 16, 8), (256, 100, 13), (400, 160, 80), (512, 256, 40), (1001, 501, 40), (1024, 256, 80), (1920, 480, 100), (2048, 512, 128),
                (68, 17, 5), (4096, 1024, 128))
GRAD_REQUIRED = ("F_1", "F_31", "F_32", "F_33", "L_255", "L_0", "L_1", "n_mel_off_8", "pad_mode_0", "pad_mode_1", "log", "linear", "zero_row",
                 "sign_pattern", "ragged", "zero_frame_short", "zero_frame_pad", "off_grid", "wave15", "generic_pass", "lds_optin", "odd_nfft")


def grad_by_id(name):
    return next(c for c in GRAD if c.id == name)


def grad_labels(c):
    out = {f"F_{c.F}", f"L_{c.L % OLA_BLOCK}", f"pad_mode_{c.pad_mode}", "log" if c.log_clip > 0 else "linear", frames_form(c.n_fft)}
    if c.n_mel % 8:
        out.add("n_mel_off_8")
    if 3 * c.hop > c.n_fft:
        out.add("hop_above_third")
    if c.zero_row is not None and c.mag_eps == 0 and c.log_clip <= 0:
        out.add("zero_row")
    if c.g == "sign":
        out.add("sign_pattern")
    if c.n_fft % 2:
        out.add("odd_nfft")
    if frames_form(c.n_fft) == "mixed" and max(prime_factors(c.n_fft)) > 13:
        out.add("generic_pass")
    lds = frames_lds_bytes(c.n_fft)
    if lds and lds > 64 * 1024:
        out.add("lds_optin")
    if c.lens is not None:
        out.add("ragged")
        for n, k in zip(c.lens[1:], c.counts()[1:]):                                   # short rows are never row 0
            if k == 0 and n > c.pad:
                out.add("zero_frame_short")
                assert truncating_row_frames(n, c.n_fft, c.hop, c.pad_mode) == 1       # the row the truncating rule gave a phantom frame
            if k == 0 and n <= c.pad:
                out.add("zero_frame_pad")
            if k > 0 and (n + 2 * c.pad - c.n_fft) % c.hop:
                out.add("off_grid")
    return out


def grad_basis32(c):
    return vo.mel_filterbank(SR, c.n_fft, c.n_mel, 0, None)


def grad_window32(c):
    return vo.hann_periodic(c.n_fft, torch.float32)


def grad_inputs(c):
    """wav [B, L] float32 (zero beyond a ragged row's length), g [B, n_mel, F] float32"""
    gen = torch.Generator().manual_seed(c.seed)
    wav = ((torch.rand(c.B, c.L, generator=gen) * 2 - 1) * 0.7).float()
    if c.zero_row is not None:
        wav[c.zero_row] = 0.0
    if c.lens is not None:
        for b, n in enumerate(c.lens):
            wav[b, n:] = 0.0
    m = torch.arange(c.n_mel, dtype=torch.float64)[None, :, None]
    f = torch.arange(c.F, dtype=torch.float64)[None, None, :]
    b = torch.arange(c.B, dtype=torch.float64)[:, None, None]
    g = 1.0 + 0.5 * torch.sin(0.37 * m + 0.11 * f + b)
    if c.g == "sign":                                                                  # what an L1 loss hands down: +-1 / numel
        g = torch.sign(torch.rand(c.B, c.n_mel, c.F, generator=gen, dtype=torch.float64) - 0.5) / (c.B * c.n_mel * c.F)
    return wav, g.float()


def mel64(y, c, linear=False):
    """[n_mel, F] of ONE utterance y [L] in fp64: the oracle's extract_mel_features where the case is its configuration, a restatement
    otherwise (reflect pad n_fft / 2 for pad_mode 1, the case's eps, the linear mel for log_clip <= 0 or `linear`)"""
    if c.pad_mode == 0 and c.log_clip == 1e-5 and c.mag_eps == 1e-9 and not linear:
        return vo.extract_mel_features(y[None], c.pp, dtype=torch.float64)
    yp = Fn.pad(y[None, None], (c.pad, c.pad), mode="reflect")[0, 0]
    fr = yp.unfold(-1, c.n_fft, c.hop) * grad_window32(c).double()
    X = torch.fft.rfft(fr, dim=-1).transpose(0, 1)
    mag = torch.sqrt(X.real ** 2 + X.imag ** 2 + c.mag_eps)
    mel = torch.from_numpy(grad_basis32(c)).double() @ mag
    return mel if (linear or c.log_clip <= 0) else torch.log(torch.clamp(mel, min=c.log_clip))


def grad_reference(c, wav, g):
    """fp64 gradient [B, L], per utterance cut to its own length; zero rows for zero-frame utterances and beyond each length"""
    out = torch.zeros(c.B, c.L, dtype=torch.float64)
    lens = c.lens or [c.L] * c.B
    for b, (n, k) in enumerate(zip(lens, c.counts())):
        if k == 0 or b == c.zero_row:
            continue
        y = wav[b, :n].double().clone().requires_grad_(True)
        lm = mel64(y, c)
        assert lm.shape == (c.n_mel, k), (c.id, lm.shape, k)
        (g[b, :, :k].double() * lm).sum().backward()
        out[b, :n] = y.grad
    return out


def grad_clip_margin(c, wav):
    """smallest |mel - clip| / clip over the fp64 linear mel energies of every utterance (cases with log_clip > 0)"""
    worst = math.inf
    lens = c.lens or [c.L] * c.B
    for b, (n, k) in enumerate(zip(lens, c.counts())):
        if k:
            mel = mel64(wav[b, :n].double(), c, linear=True)
            worst = min(worst, float(((mel - c.log_clip).abs() / c.log_clip).min()))
    return worst


GRAD_MUTANTS = ("no_left_reflection", "no_right_reflection", "wk_dropped", "truncating_count")


def grad_model(c, wav, g, mutant=None):
    """float32 restatement of amp_mel_backward fed what a float32 forward returns: mel_grad_spec_kernel (the clamp's 0 / 1, B^T, wk, the
    mag > 0 guard), N irfft(H) * window, and mel_grad_ola_kernel's three reflected positions and frame range.  Frames at and beyond a row's
    own count are NaN in every input, as the GPU test poisons them."""
    n, hop, pad, F = c.n_fft, c.hop, c.pad, c.F
    lens = c.lens or [c.L] * c.B
    w64 = grad_window32(c).double().numpy()
    basis = grad_basis32(c)
    nyq = -1 if n % 2 else n // 2
    out = np.zeros((c.B, c.L), np.float32)
    for b, (Li, Fi) in enumerate(zip(lens, c.counts())):
        mel = np.full((c.n_mel, F), np.nan, np.float32)
        mag = np.full((c.bins, F), np.nan, np.float32)
        re, im = mag.copy(), mag.copy()
        gb = g[b].numpy().copy()
        gb[:, Fi:] = np.nan
        if Fi:
            y = wav[b, :Li].double().numpy()
            yp = np.pad(y, (pad, pad), mode="reflect")
            fr = np.stack([yp[f * hop:f * hop + n] for f in range(Fi)]) * w64
            X = np.fft.rfft(fr, axis=-1).T                                            # [bins, Fi]
            re[:, :Fi], im[:, :Fi] = X.real, X.imag
            mag[:, :Fi] = np.sqrt(re[:, :Fi].astype(np.float64) ** 2 + im[:, :Fi].astype(np.float64) ** 2 + c.mag_eps)
            mel[:, :Fi] = basis.astype(np.float64) @ mag[:, :Fi].astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            gm = np.where(mel >= np.float32(c.log_clip), gb / mel, np.float32(0)) if c.log_clip > 0 else gb
            acc = (basis.T.astype(np.float64) @ gm.astype(np.float64)).astype(np.float32)  # [bins, F]
            wk = np.full((c.bins, 1), 1.0 if mutant == "wk_dropped" else 0.5, np.float32)
            wk[0] = 1.0
            if nyq >= 0:
                wk[nyq] = 1.0
            s = np.where(mag > 0, wk * acc / mag, np.float32(0))
            H = (s * re).astype(np.float64) + 1j * (s * im).astype(np.float64)
        H[0] = H[0].real
        if nyq >= 0:
            H[nyq] = H[nyq].real
        full = np.zeros((n, F), complex)
        full[:c.bins] = H
        for k in range(1, c.bins):
            if k != nyq:
                full[n - k] = np.conj(H[k])
        frames = (np.fft.ifft(full, axis=0).real * n * w64[:, None]).astype(np.float32).T.copy()   # [F, n_fft]
        Fu = min(F, truncating_row_frames(Li, n, hop, c.pad_mode)) if mutant == "truncating_count" else Fi
        s_ = np.arange(Li)
        pos = [s_ + pad,
               np.where((s_ >= 1) & (s_ <= pad), pad - s_, -1),
               np.where((s_ <= Li - 2) & (2 * (Li - 1) - s_ < Li + pad), pad + 2 * (Li - 1) - s_, -1)]
        if mutant == "no_left_reflection":
            pos[1][:] = -1
        if mutant == "no_right_reflection":
            pos[2][:] = -1
        acc = np.zeros(Li, np.float32)
        for t in pos:
            ok = t >= 0
            ts = np.where(ok, t, 0)
            fa = np.where(ts - n + 1 <= 0, 0, (ts - n + hop) // hop)
            fz = np.where(ok, np.minimum(ts // hop, Fu - 1), -1)
            acc = acc + _gather_ola(frames, ts, fa, fz, hop)
        out[b, :Li] = acc
    return out


def grad_excess(c, ref, out, rule=None):
    """largest error / bound over the rows that have frames; inf where a zero-frame row, a column beyond a length or the all-zero row is
    not exactly 0, or anything is not finite.  smooth g: max |err| <= 1e-4 max |ref|; the sign pattern: max 2e-3 and mean 2e-5 of scale"""
    out = torch.as_tensor(np.asarray(out)).double() if not isinstance(out, torch.Tensor) else out.detach().cpu().double()
    if out.shape != ref.shape or not bool(torch.isfinite(out).all()):
        return math.inf
    lens = c.lens or [c.L] * c.B
    worst = 0.0
    for b, (n, k) in enumerate(zip(lens, c.counts())):
        if k == 0 or b == c.zero_row:
            if bool((out[b] != 0).any()):
                return math.inf
            continue
        if bool((out[b, n:] != 0).any()):
            return math.inf
        scale = float(ref[b].abs().max())
        err = (out[b] - ref[b]).abs()
        if (rule or c.g) == "sign":
            worst = max(worst, float(err.max()) / (SIGN_MAX * scale), float(err[:n].mean()) / (SIGN_MEAN * scale))
        else:
            worst = max(worst, float(err.max()) / (GRAD_REL * scale))
    return worst


# ------------------------------------------------------------------------------------------------------------------------------
# ragged forward, every kernel form, a hop above n_fft / 3 where the form takes one: (n_fft, hop, n_mel, the form launch_mel takes)
# ------------------------------------------------------------------------------------------------------------------------------
RAGGED_FWD = [(1024, 512, 80, "mel1024"), (2048, 1024, 128, "mel_wave"), (512, 256, 40, "mel_wave"), (1920, 960, 100, "mel_wave"),
              (1920, 641, 100, "mel_mixed"),          # an odd hop: the wave form falls back
              (256, 100, 13, "mel_kernel"), (400, 160, 80, "mel_mixed"), (1001, 501, 40, "mel_mixed")]


def ragged_fwd_lens(n_fft, hop):
    """row 0 full (past one 32-frame tile); pad < len < hop; 33 frames off the hop grid; len <= pad; three frames"""
    pad = (n_fft - hop) // 2
    return [35 * hop + 5, pad + 1 + (hop - pad - 1) // 2, 33 * hop + 7, pad, 3 * hop + 1]
