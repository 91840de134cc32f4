"""TEST INFRASTRUCTURE -- a plain-torch restatement of HubertModel(wav)["last_hidden_state"] (HubertConfig() order:
GroupNorm feature encoder, post-LN layers), written from the model's definition for lengths the golden file does not hold.
CPU, fp32 by default; float64 gives the spread the fp32 device path is judged against.  Needs neither transformers nor
the reference.

    last, inter = forward(weights, config, wav)      # last [Th][H]; inter["features"] [T][C], inter["pre_ln"] [Th][H]
"""
import math

import numpy as np
import torch
import torch.nn.functional as F


def frames(config, n):
    for k, s in zip(config["conv_kernel"], config["conv_stride"]):
        if n < k:
            return 0
        n = (n - k) // s + 1
    return n


def _t(w, name, dtype):
    return torch.as_tensor(np.asarray(w[name])).to(dtype)


def forward(weights, config, wav, dtype=torch.float32):
    """weights: state dict under the weight_g / weight_v names (numpy or torch), wav [n] -> (last [Th][H], intermediates)"""
    W = lambda n: _t(weights, n, dtype)
    eps = float(config.get("layer_norm_eps", 1e-5))
    H, heads = config["hidden_size"], config["num_attention_heads"]
    x = torch.as_tensor(np.asarray(wav)).to(dtype).reshape(1, 1, -1)
    # feature encoder: conv 0 + GroupNorm(C, C) (per channel over all frames) + GELU, then conv + GELU
    for i, s in enumerate(config["conv_stride"]):
        x = F.conv1d(x, W("feature_extractor.conv_layers.%d.conv.weight" % i), stride=s)
        if i == 0:
            x = F.group_norm(x, x.shape[1], W("feature_extractor.conv_layers.0.layer_norm.weight"),
                             W("feature_extractor.conv_layers.0.layer_norm.bias"), eps=1e-5)
        x = F.gelu(x)
    feats = x[0].transpose(0, 1)                                   # [T][C]
    h = F.layer_norm(feats, feats.shape[-1:], W("feature_projection.layer_norm.weight"), W("feature_projection.layer_norm.bias"), eps)
    h = F.linear(h, W("feature_projection.projection.weight"), W("feature_projection.projection.bias"))
    # positional conv: weight norm over dims 0, 1 per tap, padding k/2, last frame dropped (even k), GELU, residual
    g, v = W("encoder.pos_conv_embed.conv.weight_g"), W("encoder.pos_conv_embed.conv.weight_v")
    wpos = v * (g / v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt())
    k = config["num_conv_pos_embeddings"]
    pos = F.conv1d(h.transpose(0, 1)[None], wpos, W("encoder.pos_conv_embed.conv.bias"), padding=k // 2,
                   groups=config["num_conv_pos_embedding_groups"])
    if k % 2 == 0:
        pos = pos[:, :, :-1]
    pre = h + F.gelu(pos[0].transpose(0, 1))
    x = F.layer_norm(pre, (H,), W("encoder.layer_norm.weight"), W("encoder.layer_norm.bias"), eps)
    T, D = x.shape[0], H // heads
    for l in range(config["num_hidden_layers"]):
        p = "encoder.layers.%d." % l
        lin = lambda t, n: F.linear(t, W(p + n + ".weight"), W(p + n + ".bias"))
        q = lin(x, "attention.q_proj").view(T, heads, D).transpose(0, 1)
        kk = lin(x, "attention.k_proj").view(T, heads, D).transpose(0, 1)
        vv = lin(x, "attention.v_proj").view(T, heads, D).transpose(0, 1)
        a = torch.softmax((q @ kk.transpose(1, 2)) * (1.0 / math.sqrt(D)), dim=-1) @ vv
        a = lin(a.transpose(0, 1).reshape(T, H), "attention.out_proj")
        x = F.layer_norm(x + a, (H,), W(p + "layer_norm.weight"), W(p + "layer_norm.bias"), eps)
        f = lin(F.gelu(lin(x, "feed_forward.intermediate_dense")), "feed_forward.output_dense")
        x = F.layer_norm(x + f, (H,), W(p + "final_layer_norm.weight"), W(p + "final_layer_norm.bias"), eps)
    return x, {"features": feats, "pre_ln": pre}
