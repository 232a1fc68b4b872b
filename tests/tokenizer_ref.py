"""fp64 / fp32 restatement of the semantic tokenizers in eval mode, written from the reference's arithmetic: RepCodec
(models/codec/kmeans/repcodec_model.py), CocoContentStyle / CocoContent / CocoStyle (models/codec/coco/rep_coco_model.py) and VevoRepCodec
(models/codec/vevo/vevo_repcodec.py).  The Vocos backbone's pieces come from vocos_ref, the factorized quantizer and its margin rule from codec_ref,
the Euclidean quantizer from speechtokenizer_ref.  Weights regenerate from seeds.  Not imported by the library."""
import math
from collections import OrderedDict
from types import SimpleNamespace

import torch
import torch.nn.functional as Fn

import codec_ref as C
import speechtokenizer_ref as S
import vocos_ref as V

QP = "quantizer.quantizers."


# ---- hyperparameters -------------------------------------------------------------------------------------------------------------------
def small_repcodec_hp(K=64, N=1):
    return dict(codebook_size=K, hidden_size=64, codebook_dim=8, vocos_dim=32, vocos_intermediate_dim=128, vocos_num_layers=2, num_quantizers=N,
                downsample_scale=1)


def recipe_repcodec_hp():
    """models/tts/maskgct/config/maskgct.json: model.semantic_codec"""
    return dict(codebook_size=8192, hidden_size=1024, codebook_dim=8, vocos_dim=384, vocos_intermediate_dim=2048, vocos_num_layers=12,
                num_quantizers=1, downsample_scale=1)


def small_coco_hp(K=64, N=1, rate=4):
    return dict(codebook_size=K, hidden_size=64, codebook_dim=8, num_quantizers=N, whisper_dim=64, chromagram_dim=24, downsample_rate=rate,
                vocos_dim=32, vocos_intermediate_dim=128, vocos_num_layers=2)


def recipe_coco_hp():
    """models/svc/vevosing/config/fm_emilia101k_singnet7k.json: model.coco"""
    return dict(codebook_size=16384, hidden_size=1024, codebook_dim=8, num_quantizers=1, whisper_dim=1024, chromagram_dim=24, downsample_rate=4,
                vocos_dim=384, vocos_intermediate_dim=2048, vocos_num_layers=12)


def coco_cfg(hp):
    """the object the Coco constructors read (utils.util.JsonHParams in the reference)"""
    voc = dict(vocos_dim=hp["vocos_dim"], vocos_intermediate_dim=hp["vocos_intermediate_dim"], vocos_num_layers=hp["vocos_num_layers"])
    return SimpleNamespace(codebook_size=hp["codebook_size"], hidden_size=hp["hidden_size"], codebook_dim=hp["codebook_dim"],
                           num_quantizers=hp["num_quantizers"], whisper_dim=hp["whisper_dim"], chromagram_dim=hp["chromagram_dim"],
                           downsample_rate=hp["downsample_rate"], encoder=SimpleNamespace(**voc), decoder=SimpleNamespace(**voc))


def small_vevo_hp(N=1):
    return dict(input_channels=64, output_channels=64, encode_channels=64, decode_channels=64, code_dim=64, codebook_num=N, codebook_size=32)


def fvq_hp(hp):
    return dict(D=hp["hidden_size"], d=hp["codebook_dim"], K=hp["codebook_size"], N=hp["num_quantizers"], l2=True)


# ---- state_dict layouts, in the reference's order --------------------------------------------------------------------------------------
def _backbone_linear_shapes(s, p, cin, hp, cout):
    vhp = dict(input_channels=cin, dim=hp["vocos_dim"], intermediate_dim=hp["vocos_intermediate_dim"], num_layers=hp["vocos_num_layers"], n_fft=16)
    for k, shp in V.vocos_param_shapes(vhp).items():
        if k.startswith("backbone."):
            s[f"{p}0.{k[len('backbone.'):]}"] = shp
    s[p + "1.weight"] = (cout, hp["vocos_dim"])
    s[p + "1.bias"] = (cout,)


def _linear(s, p, cout, cin):
    s[p + "weight"] = (cout, cin)
    s[p + "bias"] = (cout,)


def repcodec_param_shapes(hp):
    s, H = OrderedDict(), hp["hidden_size"]
    if hp["downsample_scale"] is not None and hp["downsample_scale"] > 1:
        s["down.weight"], s["down.bias"], s["up.weight"], s["up.bias"] = (H, H, 3), (H,), (H, H, 3), (H,)
    _backbone_linear_shapes(s, "encoder.", H, hp, H)
    _backbone_linear_shapes(s, "decoder.", H, hp, H)
    s.update(C.fvq_param_shapes(fvq_hp(hp), QP))
    return s


def coco_param_shapes(hp, whisper=True, chroma=True, only_quantizer=False):
    s, H = OrderedDict(), hp["hidden_size"]
    if whisper:
        _linear(s, "whisper_input_layer.", H, hp["whisper_dim"])
    if chroma:
        _linear(s, "chromagram_input_layer.", H, hp["chromagram_dim"])
    n = int(math.log2(hp["downsample_rate"]))
    for i in range(n):
        s[f"downsample_layers.{2 * i}.weight"], s[f"downsample_layers.{2 * i}.bias"] = (H, H, 3), (H,)
    for i in range(n):
        s[f"upsample_layers.{2 * i}.weight"], s[f"upsample_layers.{2 * i}.bias"] = (H, H, 4), (H,)
    _backbone_linear_shapes(s, "encoder.", H, hp, H)
    s.update(C.fvq_param_shapes(fvq_hp(hp), QP))
    if not only_quantizer:
        _backbone_linear_shapes(s, "decoder.", H, hp, H)
        if whisper:
            _linear(s, "whisper_output_layer.", hp["whisper_dim"], H)
        if chroma:
            _linear(s, "chromagram_output_layer.", hp["chromagram_dim"], H)
    return s


def vevo_param_shapes(hp):
    """the shipped geometry: two blocks of two residual units per side, every ratio and stride 1, kernel 3"""
    s = OrderedDict()
    Ci, Ce, Cd, Co, D = hp["input_channels"], hp["encode_channels"], hp["decode_channels"], hp["output_channels"], hp["code_dim"]

    def units(p, c):
        for u in range(2):
            s[f"{p}res_units.{u}.conv1.conv.weight"] = (c, c, 3)
            s[f"{p}res_units.{u}.conv2.weight"] = (c, c, 1)

    def conv(p, cout, cin, bias):
        s[p + "conv.weight"] = (cout, cin, 3)
        if bias:
            s[p + "conv.bias"] = (cout,)

    conv("encoder.conv.", Ce, Ci, False)
    for b in range(2):
        units(f"encoder.conv_blocks.{b}.", Ce)
        conv(f"encoder.conv_blocks.{b}.conv.", Ce, Ce, True)
    conv("decoder.conv1.", Cd, D, False)
    for b in range(2):
        conv(f"decoder.conv_blocks.{b}.conv.", Cd, Cd, True)
        units(f"decoder.conv_blocks.{b}.", Cd)
    conv("decoder.conv2.", Co, Cd, False)
    conv("projector.project.", D, Ce, False)
    for i in range(hp["codebook_num"]):
        p = f"quantizer.codebook.layers.{i}."
        s[p + "embed"], s[p + "cluster_size"], s[p + "embed_avg"] = (D, hp["codebook_size"]), (hp["codebook_size"],), (D, hp["codebook_size"])
    return s


# ---- seeded weights ----------------------------------------------------------------------------------------------------------------------
def _backbone_linear_weights(sd, p, cin, hp, seed):
    vhp = dict(input_channels=cin, dim=hp["vocos_dim"], intermediate_dim=hp["vocos_intermediate_dim"], num_layers=hp["vocos_num_layers"], n_fft=16)
    for k, v in V.synth_vocos_state_dict(vhp, seed).items():
        if k.startswith("backbone."):
            sd[f"{p}0.{k[len('backbone.'):]}"] = v


def _fill(shapes, seed):
    """fan-in scaled weights (a transposed conv's two taps per output), biases N(0, 0.05)"""
    g = torch.Generator().manual_seed(seed)
    sd = OrderedDict()
    for k, shp in shapes.items():
        if k.endswith("bias"):
            sd[k] = 0.05 * torch.randn(shp, generator=g)
        elif k.startswith("upsample_layers."):
            sd[k] = torch.randn(shp, generator=g) / math.sqrt(2 * shp[0])
        elif k.endswith("cluster_size"):
            sd[k] = torch.ones(shp)
        elif k.endswith("embed") or k.endswith("embed_avg") or len(shp) < 2:
            sd[k] = None                     # the backbones' vectors and the codebooks: filled by their own generators
        else:
            sd[k] = torch.randn(shp, generator=g) / math.sqrt(shp[1] * (shp[2] if len(shp) == 3 else 1))
    return sd


def _synth(shapes, hp, seed, cin):
    sd = _fill(shapes, seed)
    for i, p in enumerate(("encoder.", "decoder.")):
        if p + "1.weight" in shapes:
            _backbone_linear_weights(sd, p, cin, hp, seed + 1 + i)
    sd.update(C.synth_fvq_state_dict(fvq_hp(hp), seed + 3, QP))
    return OrderedDict((k, sd[k].float().contiguous()) for k in shapes)


def synth_repcodec_state_dict(hp, seed):
    return _synth(repcodec_param_shapes(hp), hp, seed, hp["hidden_size"])


def synth_coco_state_dict(hp, seed, **kw):
    return _synth(coco_param_shapes(hp, **kw), hp, seed, hp["hidden_size"])


def synth_vevo_state_dict(hp, seed):
    shapes = vevo_param_shapes(hp)
    sd = _fill(shapes, seed)
    cbs = S.synth_codebooks(hp["code_dim"], hp["codebook_size"], hp["codebook_num"], seed + 1, s=1.0)
    for i, cb in enumerate(cbs):
        p = f"quantizer.codebook.layers.{i}."
        sd[p + "embed"] = cb.t().contiguous()
        sd[p + "embed_avg"] = cb.t().contiguous().clone()
    return OrderedDict((k, sd[k].float().contiguous()) for k in shapes)


def synth_feats(B, T, C, seed):
    """time-major features [B, T, C]"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, T, C, generator=g).float()


# ---- the golden cases (tests/golden/make_golden_tokenizers.py) ---------------------------------------------------------------------------
GOLDEN_LENGTHS = (1, 2, 3, 5, 50, 130)


def golden_inputs(T, B=2):
    """the inputs of every golden case at length T: RepCodec's features, Coco's two, VevoRepCodec's [B, C, T]"""
    return dict(rep=synth_feats(B, T, 64, 1000 + T), whisper=synth_feats(B, T, 64, 2000 + T), chroma=synth_feats(B, T, 24, 3000 + T),
                vevo=synth_feats(B, T, 64, 4000 + T).transpose(1, 2).contiguous())


def golden_models(seed):
    """name -> (hyperparameters, state_dict) of the golden nets; rep64 and rep8192 differ in their codebooks alone"""
    out = {f"rep{K}": (small_repcodec_hp(K), synth_repcodec_state_dict(small_repcodec_hp(K), seed)) for K in (64, 8192)}
    out["coco"] = (small_coco_hp(), synth_coco_state_dict(small_coco_hp(), seed + 10))
    out["vevo"] = (small_vevo_hp(), synth_vevo_state_dict(small_vevo_hp(), seed + 20))
    return out


# ---- shared pieces ---------------------------------------------------------------------------------------------------------------------
def _P(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


def linear_cf(P, p, x):
    """nn.Linear along the channel axis of [B, C, T]"""
    y = torch.einsum("oc,bct->bot", P[p + "weight"], x)
    return y + P[p + "bias"][None, :, None] if p + "bias" in P else y


def backbone_linear(P, p, x, layers):
    """nn.Sequential(VocosBackbone, nn.Linear) on [B, C, T] -> [B, out, T] (vocos.py:720-783; vocos_ref.vocos_forward's body without the head)"""
    q = p + "0."
    C_ = P[q + "norm.weight"].shape[0]
    h = Fn.conv1d(x, P[q + "embed.weight"], P[q + "embed.bias"], padding=3)
    h = V._ln_c(h, P[q + "norm.weight"], P[q + "norm.bias"])
    for i in range(layers):
        b = f"{q}convnext.{i}."
        y = Fn.conv1d(h, P[b + "dwconv.weight"], P[b + "dwconv.bias"], padding=3, groups=C_)
        y = V._ln_c(y, P[b + "norm.weight"], P[b + "norm.bias"])
        y = Fn.gelu(linear_cf(P, b + "pwconv1.", y))
        h = h + P[b + "gamma"][None, :, None] * linear_cf(P, b + "pwconv2.", y)
    h = V._ln_c(h, P[q + "final_layer_norm.weight"], P[q + "final_layer_norm.bias"])
    return linear_cf(P, p + "1.", h)


def dsconv(w, b, x, gelu):
    y = Fn.conv1d(x, w, b, stride=2, padding=1)
    return Fn.gelu(y) if gelu else y


def dsconv_bound(w, b, x, gelu):
    """fp64 output of Conv1d(k = 3, stride 2, padding 1) [-> GELU] and the bound of each element, as codec_ref.sconv_bound and the pointwise
    tests state it: 2e-6 (|w| * |x| + |b|) + 3e-7 |ref|, the first term x 1.2 behind the GELU (|gelu'| <= 1.13) with |lin| in the second"""
    lin = Fn.conv1d(x, w, b, stride=2, padding=1)
    cond = Fn.conv1d(x.abs(), w.abs(), stride=2, padding=1) + (b.abs()[None, :, None] if b is not None else 0.0)
    if gelu:
        return Fn.gelu(lin), 1.2 * 2e-6 * cond + 3e-7 * lin.abs()
    return lin, 2e-6 * cond + 3e-7 * lin.abs()


def fvq(sd, hp, z, dtype, codes=None):
    return C.rvq_forward(sd, fvq_hp(hp), z, dtype, codes=codes, prefix=QP)


def fvq_margin_rule(sd, hp, z):
    return C.margin_rule(sd, fvq_hp(hp), z, prefix=QP)


def fvq_plain(sd, hp, z):
    """ResidualVQ.forward in eval mode with the reference's own ops and nothing else (factorized_vector_quantize.py:52-127, residual_vq.py:68-152),
    in the dtype and on the device of `sd` and `z` -- the yardstick tools/tokenizer_bench.py times.  -> (codes [N, B, T], quantized [B, D, T])"""
    f = fvq_hp(hp)
    B, D, T = z.shape
    residual, zq, out = z, 0.0, []
    for i in range(f["N"]):
        p = f"{QP}{i}."
        z_e = Fn.conv1d(residual, C.folded(sd, p + "in_project."), sd[p + "in_project.bias"])
        enc = Fn.normalize(z_e.transpose(1, 2).reshape(-1, f["d"]))
        cb = Fn.normalize(sd[p + "codebook.weight"])
        dist = enc.pow(2).sum(1, keepdim=True) - 2 * enc @ cb.t() + cb.pow(2).sum(1, keepdim=True).t()
        idx = (-dist).max(1)[1].reshape(B, T)
        q = Fn.embedding(idx, sd[p + "codebook.weight"]).transpose(1, 2)
        q = Fn.conv1d(z_e + (q - z_e), C.folded(sd, p + "out_project."), sd[p + "out_project.bias"])
        zq, residual = zq + q, residual - q
        out.append(idx)
    return torch.stack(out), zq


def repcodec_quantize_plain(sd, hp, x):
    """RepCodec.quantize in sd's dtype, on its device"""
    codes, zq = fvq_plain(sd, hp, backbone_linear(sd, "encoder.", x.transpose(1, 2), hp["vocos_num_layers"]))
    return codes, zq.transpose(1, 2)


def coco_quantize_plain(sd, hp, whisper, chroma):
    """CocoContentStyle.quantize in sd's dtype, on its device"""
    x = linear_cf(sd, "whisper_input_layer.", whisper.transpose(1, 2)) + linear_cf(sd, "chromagram_input_layer.", chroma.transpose(1, 2))
    for i in range(int(math.log2(hp["downsample_rate"]))):
        x = dsconv(sd[f"downsample_layers.{2 * i}.weight"], sd[f"downsample_layers.{2 * i}.bias"], x, True)
    codes, zq = fvq_plain(sd, hp, backbone_linear(sd, "encoder.", x, hp["vocos_num_layers"]))
    return codes, zq.transpose(1, 2)


# ---- RepCodec --------------------------------------------------------------------------------------------------------------------------
def repcodec_encoder(sd, hp, x, dtype=torch.float64):
    """x [B, T, H] -> the latent [B, H, T]"""
    return backbone_linear(_P(sd, dtype), "encoder.", x.to(dtype).transpose(1, 2), hp["vocos_num_layers"])


def repcodec_decoder(sd, hp, zq, dtype=torch.float64):
    """quantized [B, H, T] -> x_rec [B, T, H]"""
    return backbone_linear(_P(sd, dtype), "decoder.", zq.to(dtype), hp["vocos_num_layers"]).transpose(1, 2)


def repcodec_forward(sd, hp, x, dtype=torch.float64, codes=None):
    z = repcodec_encoder(sd, hp, x, dtype)
    r = fvq(sd, hp, z, dtype, codes)
    return dict(z=z, codes=r["codes"], zq=r["zq"], x_rec=repcodec_decoder(sd, hp, r["zq"], dtype), margin=r["margin"])


# ---- Coco ------------------------------------------------------------------------------------------------------------------------------
def coco_input(sd, hp, feats, dtype=torch.float64):
    """feats: dict(whisper=[B, T, Cw], chroma=[B, T, Cc]) with the keys the model has -> [B, H, T]"""
    P = _P(sd, dtype)
    x = 0.0
    for name, key in (("whisper", "whisper_input_layer."), ("chroma", "chromagram_input_layer.")):
        if name in feats:
            x = x + linear_cf(P, key, feats[name].to(dtype).transpose(1, 2))
    return x


def coco_down(sd, hp, x, dtype=torch.float64):
    P = _P(sd, dtype)
    x = x.to(dtype)
    for i in range(int(math.log2(hp["downsample_rate"]))):
        x = dsconv(P[f"downsample_layers.{2 * i}.weight"], P[f"downsample_layers.{2 * i}.bias"], x, True)
    return x


def coco_encoder(sd, hp, x, dtype=torch.float64):
    return backbone_linear(_P(sd, dtype), "encoder.", x.to(dtype), hp["vocos_num_layers"])


def coco_decoder(sd, hp, zq, dtype=torch.float64):
    return backbone_linear(_P(sd, dtype), "decoder.", zq.to(dtype), hp["vocos_num_layers"])


def coco_up(sd, hp, x, T, dtype=torch.float64):
    """the up-sampling layers and the crop / last-frame padding to T, on [B, H, T']"""
    P = _P(sd, dtype)
    x = x.to(dtype)
    for i in range(int(math.log2(hp["downsample_rate"]))):
        x = Fn.gelu(Fn.conv_transpose1d(x, P[f"upsample_layers.{2 * i}.weight"], P[f"upsample_layers.{2 * i}.bias"], stride=2, padding=1))
    if x.shape[2] >= T:
        return x[:, :, :T]
    return torch.cat([x, x[:, :, -1:].repeat(1, 1, T - x.shape[2])], dim=2)


def coco_outputs(sd, hp, x, dtype=torch.float64):
    """[B, H, T] -> dict(whisper=[B, T, Cw], chroma=[B, T, Cc]) for the output layers the model has"""
    P = _P(sd, dtype)
    out = {}
    for name, key in (("whisper", "whisper_output_layer."), ("chroma", "chromagram_output_layer.")):
        if key + "weight" in P:
            out[name] = linear_cf(P, key, x.to(dtype)).transpose(1, 2)
    return out


def coco_forward(sd, hp, feats, dtype=torch.float64, codes=None, decode=True):
    T = next(iter(feats.values())).shape[1]
    x0 = coco_input(sd, hp, feats, dtype)
    down = coco_down(sd, hp, x0, dtype)
    z = coco_encoder(sd, hp, down, dtype)
    r = fvq(sd, hp, z, dtype, codes)
    out = dict(x0=x0, down=down, z=z, codes=r["codes"], zq=r["zq"], margin=r["margin"])
    if decode:
        out["dec"] = coco_decoder(sd, hp, r["zq"], dtype)
        out["up"] = coco_up(sd, hp, out["dec"], T, dtype)
        out.update(coco_outputs(sd, hp, out["up"], dtype))
    return out


# ---- VevoRepCodec ----------------------------------------------------------------------------------------------------------------------
def _vconv(P, p, x):
    return Fn.conv1d(x, P[p + "conv.weight"], P.get(p + "conv.bias"), padding=1)


def vevo_unit(P, p, x):
    y = _vconv(P, p + "conv1.", Fn.elu(x))
    return x + Fn.conv1d(Fn.elu(y), P[p + "conv2.weight"])


def vevo_encoder(sd, hp, x, dtype=torch.float64):
    P = _P(sd, dtype)
    x = _vconv(P, "encoder.conv.", x.to(dtype))
    for b in range(2):
        for u in range(2):
            x = vevo_unit(P, f"encoder.conv_blocks.{b}.res_units.{u}.", x)
        x = _vconv(P, f"encoder.conv_blocks.{b}.conv.", x)
    return x


def vevo_projector(sd, hp, x, dtype=torch.float64):
    return _vconv(_P(sd, dtype), "projector.project.", x.to(dtype))


def vevo_decoder(sd, hp, zq, dtype=torch.float64):
    P = _P(sd, dtype)
    x = _vconv(P, "decoder.conv1.", zq.to(dtype))
    for b in range(2):
        x = _vconv(P, f"decoder.conv_blocks.{b}.conv.", x)
        for u in range(2):
            x = vevo_unit(P, f"decoder.conv_blocks.{b}.res_units.{u}.", x)
    return _vconv(P, "decoder.conv2.", x)


def vevo_codebooks(sd, hp):
    """each level's rows [K, D] (VectorQuantize.codebook = embed.t())"""
    return [sd[f"quantizer.codebook.layers.{i}.embed"].t().contiguous() for i in range(hp["codebook_num"])]


def vevo_quantize(sd, hp, z, dtype=torch.float64, codes=None):
    """the levels' walk on z [B, D, T]: vevo_repcodec.py's distance is speechtokenizer_ref.evq_distances' expression.  -> evq_forward's dict
    plus the two scalars of ResidualVQ.forward (loss [N], perplexity [N])"""
    cbs = vevo_codebooks(sd, hp)
    r = S.evq_forward(cbs, z, dtype, codes=codes)
    residual, losses, perps = z.to(dtype), [], []
    for i in range(len(cbs)):
        losses.append(Fn.mse_loss(r["all_q"][i], residual))
        probs = torch.bincount(r["codes"][i].flatten(), minlength=hp["codebook_size"]).to(dtype) / r["codes"][i].numel()
        perps.append(torch.exp(-torch.sum(probs * torch.log(probs + 1e-10))))
        residual = residual - r["all_q"][i]
    r["loss"], r["perplexity"] = torch.stack(losses), torch.stack(perps)
    return r


def vevo_forward(sd, hp, x, dtype=torch.float64, codes=None):
    e = vevo_encoder(sd, hp, x, dtype)
    z = vevo_projector(sd, hp, e, dtype)
    r = vevo_quantize(sd, hp, z, dtype, codes)
    return dict(e=e, z=z, codes=r["codes"], zq=r["zq"], y=vevo_decoder(sd, hp, r["zq"], dtype), loss=r["loss"], perplexity=r["perplexity"],
                margin=r["margin"])
