"""CPU reference of ControlNet (Zhang et al. 2023) as sgm's ControlNet / ControlledUnetModel and the diffusers ControlNetModel define it, restated in
the oracle's naming and built on the oracle's own modules (imported, not modified): the parameter enumeration, the control forward and the
controlled UNet forward.

  parameters   the UNet's embeddings, input entries and middle block (names, shapes, order its own), then input_hint_block.{0..7} (3x3 pad-1
               convolutions hint_in -> hc0 -> hc0 -> hc1 -> hc1 -> hc2 -> hc2 -> hc3 -> model_channels, numbers 2, 4 and 6 with stride 2, SiLU behind
               the first seven), zero_convs.{i} (1x1, c_i -> c_i, one per input entry) and middle_block_out (1x1).  Synthetic weights: the oracle's
               recipe at gain 1.0, except the hint convolutions' weights at HINT_GAIN (at 1.0 the SiLU chain shrinks the hint features until the hint
               no longer matters: tests/test_cpu_controlnet.py holds the fixture to "it matters").
  control      g = input_hint_block(hint); h = x; per input entry i: h = input_blocks[i](h), h += g behind entry 0, r_i = zero_convs[i](h);
               r_mid = middle_block_out(middle_block(h))
  controlled   the encoder unchanged, h = middle(h) + s r_mid, every output block concatenates hs.pop() + s r.pop()
"""
import torch

from oracle import config as OC, model as OM

HINT_CHANNELS = (16, 32, 96, 256)
HINT_IN = 3
HINT_GAIN = 1.5
HINT_STRIDE2 = (2, 4, 6)


def _c_out(b):
    return b["c_out"] if "c_out" in b else b["c"]


def controlnet_param_specs(cfg, hint_in=HINT_IN, hint_channels=HINT_CHANNELS):
    s = OC._Spec()
    mc, emb = cfg.model_channels, 4 * cfg.model_channels
    s.linear("lin1_time_embed", mc, emb)
    s.linear("lin2_time_embed", emb, emb)
    s.linear("lin1_label_embed", cfg.adm_in_channels, emb)
    s.linear("lin2_label_embed", emb, emb)
    inp, mid, _ = OC.unet_block_plan(cfg)
    for i, b in enumerate(inp):
        OC._block_params(s, f"input_blocks.{i}", b, cfg.context_dim)
    OC._res_block(s, "middle_block.res1", mid["c"], mid["c_emb"], mid["c"])
    OC._transformer(s, "middle_block.transformer", mid["c"], cfg.context_dim, mid["depth"])
    OC._res_block(s, "middle_block.res2", mid["c"], mid["c_emb"], mid["c"])
    hc = tuple(hint_channels)
    chans = (hint_in, hc[0], hc[0], hc[1], hc[1], hc[2], hc[2], hc[3], mc)
    for k in range(8):
        s.conv(f"input_hint_block.{k}", chans[k], chans[k + 1], 3, gain=HINT_GAIN)
    for i, b in enumerate(inp):
        s.conv(f"zero_convs.{i}", _c_out(b), _c_out(b), 1)
    s.conv("middle_block_out", mid["c"], mid["c"], 1)
    return s.items


def control_weights(cfg, seed=1):
    return OM.to_torch(OC.synth_weights(controlnet_param_specs(cfg), seed))


def skip_shapes(cfg, H, W):
    """(C, h, w) of every residual tensor on an H x W latent: one per input entry, then the middle block's"""
    inp, mid, _ = OC.unet_block_plan(cfg)
    out, h, w = [], H, W
    for b in inp:
        if b["kind"] == "Down":
            h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        out.append((_c_out(b), h, w))
    out.append((mid["c"], h, w))
    return out


def block_hint(B, H8, W8, seed):
    """a hint of 16 x 16 blocks of zeros and ones, [B, 3, H8, W8]"""
    g = torch.Generator().manual_seed(seed)
    small = (torch.rand(B, 3, H8 // 16, W8 // 16, generator=g) > 0.5).float()
    return small.repeat_interleave(16, dim=2).repeat_interleave(16, dim=3)


def _emb(cfg, W, timesteps, label):
    t_emb = OM.timestep_embedding(timesteps, cfg.model_channels, 10000)
    t_emb = OM.linear(OM.silu(OM.linear(t_emb, W, "lin1_time_embed")), W, "lin2_time_embed")
    l_emb = OM.linear(OM.silu(OM.linear(label, W, "lin1_label_embed")), W, "lin2_label_embed")
    return OM.NUM.r(t_emb + l_emb)


def _middle(x, emb, context, W, mid):
    x = OM.res_block(x, emb, W, "middle_block.res1")
    x = OM.spatial_transformer(x, context, W, "middle_block.transformer", mid["n_head"], mid["depth"])
    return OM.res_block(x, emb, W, "middle_block.res2")


def embed_hint(W, hint):
    g = hint
    for k in range(8):
        g = OM.conv2d(g, W, f"input_hint_block.{k}", stride=2 if k in HINT_STRIDE2 else 1, padding=1)
        if k < 7:
            g = OM.silu(g)
    return g


def control_forward(cfg, W, x, timesteps, context, label, hint):
    """-> [r_0 ... r_{n_in - 1}, r_mid]"""
    inp, mid, _ = OC.unet_block_plan(cfg)
    emb = _emb(cfg, W, timesteps, label)
    g = embed_hint(W, hint)
    h, res = x, []
    for i, b in enumerate(inp):
        h = OM._unet_block(h, emb, context, W, f"input_blocks.{i}", b)
        if i == 0:
            h = h + g
        res.append(OM.conv2d(h, W, f"zero_convs.{i}", cls="conv_skip"))
    h = _middle(h, emb, context, W, mid)
    res.append(OM.conv2d(h, W, "middle_block_out", cls="conv_skip"))
    return res


def controlled_unet_forward(cfg, W, x, timesteps, context, label, residuals=None, scale=1.0):
    """OM.unet_forward with scale * residuals added to the middle block's output and to every skip tensor the decoder concatenates (residuals=None:
    the same operations as OM.unet_forward, bit for bit)"""
    inp, mid, out = OC.unet_block_plan(cfg)
    x, context, label = OM.NUM.r(x), OM.NUM.r(context), OM.NUM.r(label)
    emb = _emb(cfg, W, timesteps, label)
    saved = []
    for i, b in enumerate(inp):
        x = OM._unet_block(x, emb, context, W, f"input_blocks.{i}", b)
        saved.append(x)
    x = _middle(x, emb, context, W, mid)
    res = None
    if residuals is not None:
        res = list(residuals)
        assert len(res) == len(inp) + 1
        x = x + scale * res.pop()
    for i, b in enumerate(out):
        skip = saved.pop()
        if res is not None:
            skip = skip + scale * res.pop()
        x = torch.cat([x, skip], dim=1)
        x = OM._unet_block(x, emb, context, W, f"output_blocks.{i}", b)
    x = OM.silu(OM.gn(x, W, "norm_out"))
    return OM.conv2d(x, W, "conv_out", padding=1, cls="conv_io")

