"""The range guard at generator level: an operand that first leaves the split-f16 range INSIDE a whole-resblock kernel, deep in
the network, and an out-of-range batch that goes through the drop-in entry point's cached hipGraph.

tests/test_gpu_range_guard.py drives conv_pre's output out of range with a mel spike: the first launch of the forward catches it.
Here one deep layer is scaled instead (resblocks.3.convs2.0, the first pair of stage 1), so that the operand that leaves the range is
the x a whole-resblock kernel builds in registers for its second pair; and the graph path (``_forward_graphed_view``: replayed with
``replay(check=False)``, no flag copy while capturing) must still report it, fall back to the exact-fp32 kernels and keep no f16x3
graph behind."""
import warnings
from types import SimpleNamespace as NS

import pytest
import torch

from oracle import synth
from oracle import vocoder_oracle as vo

pytestmark = pytest.mark.gpu

DEEP = "resblocks.3.convs2.0.weight_g"          # stage 1 (C = 32 at upsample_initial_channel 128), resblock 0, pair 0's second conv


@pytest.fixture(autouse=True)
def _f16x3_and_policy():
    from amphion_amd import _lib

    _lib.set_precision("f16x3")
    yield
    _lib.set_precision("f16x3")
    _lib.check(_lib.lib().amp_set_resblock_fusion(-1))


def _hifigan(scale=1.0):
    from amphion_amd.models.vocoders.gan.generator.hifigan import HiFiGAN

    hp = dict(vo.hifigan_v1_hp(), upsample_initial_channel=128)
    m = HiFiGAN(NS(preprocess=NS(n_mel=80, hop_size=256, extract_amplitude_phase=False), model=NS(hifigan=NS(**hp))))
    sd = synth.synth_state_dict(synth.hifigan_param_shapes(80, hp), 1234)
    sd[DEEP] = sd[DEEP] * scale
    m.load_state_dict(sd)
    return m.cuda().eval(), sd, hp


def _rb_waves(m):
    """waves (WM * WN) of the whole-resblock kernels stage 1's k = 3 resblock ran in the last profiled forward"""
    names = m.kernel_names(100 + 16 * 1 + 0)
    return {int(a) * int(b) for n in names if n.startswith("rb_f16x3_kernel<") for a, b in [n.split("<")[1].split(", ")[1:3]]}


@pytest.mark.parametrize("mode,waves", [(2, 8), (3, 4)])
def test_deep_layer_beyond_the_range_inside_the_resblock_kernel(mode, waves):
    """check_range() raises, the next forward refuses without a synchronisation, forward_exact_range() warns and gives the fp64
    reference's audio; the same model unscaled never flags.  The whole-resblock kernel (both forms) is confirmed to have run."""
    from amphion_amd import _lib

    _lib.check(_lib.lib().amp_set_resblock_fusion(mode))
    mel = synth.synth_mel(1, 80, 12, seed=3)
    good, _, _ = _hifigan()
    with torch.no_grad():
        good.set_profiling(1)
        good(mel.cuda())
        good.check_range()                                   # unscaled: nothing leaves the range
        assert _rb_waves(good) == {waves}, good.kernel_names(116)

    # x 1e4: the x entering pair 1 of that resblock is 2.2e4 in fp64 (5x the 4094 limit; x 1e3 stays at 2 195, in range), and every
    # operand before it is below 12
    m, sd, hp = _hifigan(1e4)
    ref = vo.hifigan_forward(sd, hp, mel, dtype=torch.float64)
    ref32 = vo.hifigan_forward(sd, hp, mel, dtype=torch.float32)
    with torch.no_grad():
        m.set_profiling(1)
        m(mel.cuda())
        assert _rb_waves(m) == {waves}
        with pytest.raises(_lib.AmpError) as e:
            m.check_range()
        assert e.value.status == _lib.AMP_ERR_RANGE
        m.check_range()                                      # the report cleared it
        m(mel.cuda())
        torch.cuda.synchronize()
        with pytest.raises(_lib.AmpError) as e:              # lazy: the NEXT forward refuses
            m(mel.cuda())
        assert e.value.status == _lib.AMP_ERR_RANGE
        m.set_profiling(0)
        with pytest.warns(RuntimeWarning, match="exact-fp32"):
            y = m.forward_exact_range(mel.cuda())
    assert torch.isfinite(y).all()
    err, base = (y.cpu().double() - ref).abs().max().item(), (ref32.double() - ref).abs().max().item()
    assert err <= max(1e-4, 6 * base), (err, base)


def test_graph_cache_reports_falls_back_and_drops_f16x3_graphs():
    """vocoder_inference on one bucket: the second call replays a captured f16x3 graph.  An out-of-range batch through that graph
    is reported (the replayed kernels write the handle's word; the entry point's check reads it), warns and is redone on the
    exact-fp32 kernels; every later call of the bucket replays an fp32 graph: the eager fp32 forward's bits."""
    from amphion_amd.models.vocoders.gan.gan_vocoder_inference import vocoder_inference

    m, sd, hp = _hifigan()
    cfg = m.cfg
    good = synth.synth_mel(1, 80, 12, seed=4)
    bad = good.clone()
    bad[0, :, 6] = 1e5                                       # conv_pre's output far beyond 4094
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        a1 = vocoder_inference(cfg, m, good, device="cuda")   # eager (first sight of the bucket)
        a2 = vocoder_inference(cfg, m, good, device="cuda")   # captured and replayed
    assert torch.equal(a1, a2)
    m.check_range()                                          # in range through the graph: no flag
    ref = vo.hifigan_forward(sd, hp, bad, dtype=torch.float64)
    ref32 = vo.hifigan_forward(sd, hp, bad, dtype=torch.float32)
    with pytest.warns(RuntimeWarning, match="exact-fp32"):
        yb = vocoder_inference(cfg, m, bad, device="cuda")   # the f16x3 graph's replay flags; redone in fp32
    assert torch.isfinite(yb).all()
    err, base = (yb.double() - ref.squeeze(1)).abs().max().item(), (ref32.double() - ref).abs().max().item()
    assert err <= max(1e-4, 6 * base), (err, base)
    with torch.no_grad():
        eager32 = m(good.cuda()).squeeze(1).cpu()            # the generator is on the fp32 kernels from now on
        eager32b = m(bad.cuda()).squeeze(1).cpu()
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        outs = [vocoder_inference(cfg, m, mel, device="cuda") for mel in (good, good, good, bad)]
    for o in outs[:3]:
        assert torch.equal(o, eager32)                       # an f16x3 graph left in the cache would give other bits
    assert torch.equal(outs[3], eager32b)
    m.check_range()
