"""TEST INFRASTRUCTURE -- a plain-torch restatement of BertForMaskedLM(ids, output_hidden_states=True).hidden_states[-3]
for one text (absolute positions, token type 0, no mask, post-LN layers) and of CNRoberta's phone expansion, written from
the model's definition for lengths and batches the golden file does not hold.  CPU, fp32 by default; float64 gives the
spread the fp32 device path is judged against.  Needs neither transformers nor the reference.

    hid = forward(weights, config, ids)          # [len(ids)][H], hidden_states[-3] of that text
    ph = expand(hid, word2ph["ph"])             # rows 1 .. len-2 repeated by ph
"""
import math

import numpy as np
import torch
import torch.nn.functional as F


def _t(w, name, dtype):
    return torch.as_tensor(np.asarray(w[name])).to(dtype)


def forward(weights, config, ids, dtype=torch.float32):
    """weights: state dict without the "bert." prefix (numpy or torch), ids [T] with [CLS] / [SEP] -> [T][H]"""
    W = lambda n: _t(weights, n, dtype)
    eps = float(config.get("layer_norm_eps", 1e-12))
    H, heads = config["hidden_size"], config["num_attention_heads"]
    ids = torch.as_tensor(list(ids), dtype=torch.int64)
    T, D = ids.numel(), H // heads
    x = W("embeddings.word_embeddings.weight")[ids] + W("embeddings.token_type_embeddings.weight")[0]
    x = x + W("embeddings.position_embeddings.weight")[:T]
    x = F.layer_norm(x, (H,), W("embeddings.LayerNorm.weight"), W("embeddings.LayerNorm.bias"), eps)
    for l in range(config["num_hidden_layers"] - 2):
        p = "encoder.layer.%d." % l
        lin = lambda t, n: F.linear(t, W(p + n + ".weight"), W(p + n + ".bias"))
        q = lin(x, "attention.self.query").view(T, heads, D).transpose(0, 1)
        k = lin(x, "attention.self.key").view(T, heads, D).transpose(0, 1)
        v = lin(x, "attention.self.value").view(T, heads, D).transpose(0, 1)
        a = torch.softmax((q @ k.transpose(1, 2)) / math.sqrt(D), dim=-1) @ v
        a = lin(a.transpose(0, 1).reshape(T, H), "attention.output.dense")
        x = F.layer_norm(a + x, (H,), W(p + "attention.output.LayerNorm.weight"), W(p + "attention.output.LayerNorm.bias"), eps)
        f = lin(F.gelu(lin(x, "intermediate.dense")), "output.dense")
        x = F.layer_norm(f + x, (H,), W(p + "output.LayerNorm.weight"), W(p + "output.LayerNorm.bias"), eps)
    return x


def expand(hidden, ph):
    """CNRoberta: drop [CLS] / [SEP], repeat_interleave by word2ph["ph"] -> [sum(ph)][H]"""
    return torch.repeat_interleave(hidden[1:-1], torch.as_tensor(list(ph), dtype=torch.int64), dim=0)
