"""Op-level parity at the layer shapes of the recipe vocoders (tests/recipe_shapes.py): every distinct conv_pre, ConvTranspose1d,
resblock conv and conv_post of BigVGAN-large, the 100-mel TFR-enhanced HiFi-GAN, the NSF-HiFiGAN recipe and the resblock-2 HiFi-GAN
recipe, through the C ABI (amp_conv_forward), at two grids each:
  small  one short utterance (B = 1): the half-width tiles and the whole-K conv_small kernel;
  large  B = 4 at the smallest length (x 1.25) at which the launch policy picks its large-grid form: the row-blocked conv_blk kernel
         where the layer has one, else the full-width conv_f16x3 tiles.
Each output is compared with the fp64 windowed reference (tests/conv_window_ref.py) on probe rows (the first and last row of every
GEMM row group, the last real row next to the padding, random rows) x column windows (both ends, tile seams, a random spot) of items
0 and B - 1, as |hip - fp64| / cond <= BOUND (tests/test_recipe_numerics.py derives it and shows that a kernel that lost one of the
three split-f16 products exceeds it at every one of these shapes).

Which kernel ran is asserted, not inferred: the cases of a group run in ONE child process with AMP_LAUNCH_MANIFEST set, and each case
must have launched exactly the kernel recipe_shapes.Op.form() names for it (conv_blk with its tap count, its waves along the columns
and its grid order: /2d is the 2-D grid, /1d the row-group-fastest order).  Between them the cases reach
  conv_blk with several row groups in the 2-D grid (C = 768: 7 MB of weights > the 3 MB of the 1-D order), k = 3 and ConvT (kt2),
  the A-ring conv_blk at k = 7 and 11 (C = 768), the narrow 128-row conv_blk (C = 384, k = 7 / 11; C = 128 k = 7 d = 3),
  conv_f16x3 with padded rows (C = 192 / 96 / 48 / 24, ConvT rows 192 / 96 / 48, conv_post's single row),
  conv_small with padded rows (C = 192 / 96 in one utterance), and conv_mfma (every case in f32 mode);
test_recipe_numerics.py::test_recipe_cases_reach_every_form checks that the table names each of them.  No listed form is unreachable.
conv_blk never has padded rows: the policy takes it only for M % 256 == 0 (or M % 128 == 0, narrow).

act1d (snakebeta, logscale) runs at every stage width of BigVGAN-large against the oracle's Activation1d in fp64."""
import json
import os
import subprocess
import sys
import traceback

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from recipe_shapes import Op, recipe_ops  # noqa: E402

BOUND = 2e-6          # |hip - fp64| / cond: the derivation is in tests/test_recipe_numerics.py (test_bound_separates_three_from_two_terms)
ACT_BOUND = 5e-6      # act1d, max-abs against fp64 (the bound of tests/test_gpu_bigvgan.py)


def small_grid(op):
    """(B, T) of one short utterance at this layer: 40 frames into conv_pre, 150 into a ConvT, 600 samples elsewhere"""
    if op.cin in (80, 100):
        return 1, 40
    return 1, 150 if op.u else 600


def large_grid(op):
    """(B, T): B = 4 at 1.25 x the smallest length at which the policy takes its large-grid form: conv_blk where the layer reaches it
    at any length, else the full-width conv_f16x3 tiles"""
    B = 4

    def large(T):
        f, _, tile = op.form(B, T)
        return f.startswith("conv_blk") or (f == "conv_f16x3_kernel" and tile == 128 * (4 // op.WM) * (op.u or 1))

    blk = op.form(B, 1 << 18)[0].startswith("conv_blk")
    T0 = next(T for T in range(16, 1 << 18, 16) if large(T) and (not blk or op.form(B, T)[0].startswith("conv_blk")))
    T = int(T0 * 1.25) + 7
    assert large(T) and op.form(B, T)[0] == op.form(B, T0)[0], op
    return B, T


def cases():
    """[(case id, Op, recipes)] in a fixed order"""
    ops = recipe_ops()
    order = sorted(ops, key=lambda o: (o.u > 0, -o.cin, o.cout, o.k, o.d, o.u))
    return [(op.name, op, ops[op]) for op in order]


def _epilogue(op):
    """the on-load / epilogue variant of this layer in the generator: resblock convs run lrelu-on-load; c2 (d = 1) adds the residual,
    the dilated c1 applies the next lrelu on the way out; ConvT and conv_post read lrelu(x) (slopes 0.1 / 0.01)"""
    if op.u:
        return dict(slope_in=0.1)
    if op.cout == 1:
        return dict(slope_in=0.01)
    if op.cin in (80, 100):
        return {}
    if op.d == 1:
        return dict(slope_in=0.1, res=True)
    return dict(slope_in=0.1, slope_out=0.1)


_NOISE = {}


def _noise(n, seed):
    """n standard normal values (cached per seed: one draw serves every case of a child)"""
    buf = _NOISE.get(seed)
    if buf is None or buf.numel() < n:
        g = torch.Generator().manual_seed(seed)
        buf = torch.randn(max(n, 1 << 22), generator=g)
        _NOISE[seed] = buf
    return buf[:n]


# ------------------------------------------------------------------------------------------------------------------------------
# child side
# ------------------------------------------------------------------------------------------------------------------------------
def run_conv_case(op, grid, precision):
    """one layer at one grid: returns the largest error ratio; raises AssertionError above BOUND"""
    from conv_window_ref import conv_window, error_ratio, pick, probe_rows, probe_windows
    from hip_helpers import conv_forward

    B, T = small_grid(op) if grid == "small" else large_grid(op)
    g = torch.Generator().manual_seed(op.cin * 131 + op.cout * 7 + op.k * 3 + op.d + op.u)
    if op.u:
        w = torch.randn(op.cin, op.cout, op.k, generator=g) * (op.cin * op.k / op.u) ** -0.5
    else:
        w = torch.randn(op.cout, op.cin, op.k, generator=g) * (op.cin * op.k) ** -0.5
    b = torch.randn(op.cout, generator=g) * 0.1
    x = _noise(B * op.cin * T, 1).view(B, op.cin, T)
    ep = dict(_epilogue(op))
    Tout = op.out_len(T)
    res = _noise(B * op.cout * Tout, 2).view(B, op.cout, Tout) if ep.pop("res", False) else None
    y = conv_forward(w, b, x, res=res, **op.kwargs(), **ep)
    assert y.shape == (B, op.cout, Tout), y.shape
    assert torch.isfinite(y).all()
    _, rows_per_group, tile = op.form(B, T, precision)
    rows = probe_rows(op.cout, rows_per_group, up=op.u or 1, seed=op.cin + op.k)
    wins = probe_windows(Tout, tile or 128, seed=op.cout + op.d)
    items = sorted({0, B - 1})
    ref, cond, cols = conv_window(x, w, b, rows=rows, windows=wins, items=items, res=res, **op.kwargs(), **ep)
    r = error_ratio(pick(y, items, rows, cols), ref, cond)
    assert r <= BOUND, f"{op.name} {grid} B={B} T={T}: |hip - fp64| / cond = {r:.3e} > {BOUND:g}"
    return r


def run_act_case(C, B, T):
    from hip_helpers import act1d_forward
    from oracle import vocoder_oracle as vo

    g = torch.Generator().manual_seed(C + T)
    x = torch.randn(B, C, T, generator=g) * 1.5
    al = torch.randn(C, generator=g) * 0.3
    be = torch.randn(C, generator=g) * 0.3
    f = vo.kaiser_sinc_filter1d(0.25, 0.3, 12)
    y = act1d_forward(x, al, be, True, f, f)
    ref = vo.activation1d(x.double(), al.double(), be.double(), True, f.double(), f.double())
    err = (y.double() - ref).abs().max().item()
    assert err <= ACT_BOUND, f"act1d C={C} B={B} T={T}: max |hip - fp64| = {err:.3e} > {ACT_BOUND:g}"
    return err


ACT_CASES = [(768, 2, 2056), (384, 2, 4100), (192, 1, 1025), (96, 1, 3080), (48, 1, 2048), (24, 2, 12290)]


def group_cases(group, precision):
    """[(case id, callable returning the error ratio, the kernel ids its launches must name)]"""
    if group == "act1d":
        return [(f"act1d_C{C}_B{B}_T{T}", (lambda C=C, B=B, T=T: run_act_case(C, B, T)), {"act1d_kernel"}) for C, B, T in ACT_CASES]
    out = []
    for name, op, _ in cases():
        B, T = small_grid(op) if group == "small" else large_grid(op)
        out.append((f"{name}/{group}", (lambda op=op: run_conv_case(op, group, precision)), {op.form(B, T, precision)[0]}))
    return out


def _kernel_id(line):
    """manifest line -> kernel id: conv_blk gets /k<KT>/wn<WN>/<1d|2d> (the grid order from the line's grid=XxY)"""
    name, what = line.split("\t")[0], line.split("\t")[-1]
    base = name.split("<")[0]
    if base == "conv_blk_kernel":                     # <KT, NI, HALO, CM, RING, WN>
        args = [int(v) for v in name.split("<")[1].rstrip(">").split(",")]
        gy = int(what.rsplit("grid=", 1)[1].split("x")[1])
        return f"{base}/k{args[0]}/wn{args[5]}/{'2d' if gy > 1 else '1d'}"
    return base


def _child(group, precision, out, cases_fn=None):
    """run the group's cases in order (cases_fn: another table of the same form, tests/test_gpu_conv_geometry.py).
    Only a failed assertion moves on to the next case: any other error (a failed launch, a
    HIP error) ends the process at once, after recording what was done, so nothing more is started on a device in doubt."""
    sys.path.insert(0, ROOT)
    torch.set_num_threads(16)
    from amphion_amd import _lib

    _lib.set_precision(precision)
    man = os.environ["AMP_LAUNCH_MANIFEST"]
    res = {}
    for name, fn, _ in (cases_fn or group_cases)(group, precision):
        n0 = sum(1 for _ in open(man)) if os.path.exists(man) else 0
        err, fatal, ratio = None, None, None
        try:
            ratio = fn()
        except AssertionError:
            err = traceback.format_exc()[-3000:]
        except BaseException as e:
            err, fatal = traceback.format_exc()[-3000:], e
        lines = open(man).read().splitlines()[n0:] if os.path.exists(man) else []
        res[name] = {"err": err, "ratio": ratio, "kernels": sorted({_kernel_id(l) for l in lines}),
                     "launches": [l.split("\t")[-1] for l in lines]}
        with open(out, "w") as fh:                # after every case: an early end leaves what was done
            json.dump(res, fh)
        if fatal is not None:
            raise fatal


# ------------------------------------------------------------------------------------------------------------------------------
# parent side: ONE test per (group, precision), so that each child process starts exactly once whatever the number of workers
# ------------------------------------------------------------------------------------------------------------------------------
def _run_group(group, precision, tmp_path, cases_fn=None, script=None, title="recipe shapes", bound=None):
    """bound: what a case's figure is printed against (default: the conv bound, ACT_BOUND for act1d); 1 for cases that return error / bound"""
    out, man = tmp_path / "results.json", tmp_path / "manifest.tsv"
    env = dict(os.environ, AMP_LAUNCH_MANIFEST=str(man), AMP_PRECISION=precision)
    r = subprocess.run([sys.executable, os.path.abspath(script or __file__), group, precision, str(out)], capture_output=True, text=True,
                       env=env, timeout=900)
    res = json.load(open(out)) if out.exists() else {}
    problems, table = [], []
    if bound is None:
        bound = ACT_BOUND if group == "act1d" else BOUND
    for name, _, kernels in (cases_fn or group_cases)(group, precision):
        if name not in res:
            problems.append(f"{name}: not run (the child ended first)")
            continue
        c = res[name]
        if c["err"] is not None:
            problems.append(f"{name}:\n{c['err']}")
        if set(c["kernels"]) != kernels:
            problems.append(f"{name}: ran {c['kernels']}, not {sorted(kernels)}")
        ratio = c["ratio"]
        table.append(f"{precision:6s} {name:34s} {' + '.join(c['kernels']):34s} "
                     f"{'-' if ratio is None else f'{ratio / bound:.3f}':>7s}  {' | '.join(c['launches'])}")
    print(f"\n# {title}, group {group}, {precision}: case, kernels, largest error / bound ({bound:g}), launch\n" + "\n".join(table))
    assert r.returncode == 0 and not problems, f"child exit {r.returncode}\n" + "\n".join(problems) + "\n" + r.stderr[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("group", ["small", "large"])
def test_recipe_conv_shapes(group, conv_precision, tmp_path):
    _run_group(group, conv_precision, tmp_path)


@pytest.mark.gpu
def test_recipe_act1d_widths(tmp_path):
    """act1d has no conv contraction and no precision switch: one run"""
    _run_group("act1d", "f16x3", tmp_path)


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2], sys.argv[3])
