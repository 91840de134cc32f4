"""CPU: this package's loader against what the reference's own Loader (gsv_tts/Loader.py:59-170, nn.Modules on the CPU)
makes of the SAME checkpoint files, recorded in tests/golden/loader.json + loader.npz by oracle/gen_golden.py (`loader`):
the resulting state must agree tensor for tensor.  This pins SURVEY.md 8(a) row a3 to the reference instead of to the
package's own key map: the GPT file below spells the UPSTREAM names out literally, and the SoVITS file carries the
reference module's own state dict layout (weight-normed Generator and flow, as upstream checkpoints are).

What the fixture holds, per case: GPT -- the config and, for every key of the reference's module, the upstream key whose
tensor it holds bit for bit; SoVITS -- the reference module's state-dict manifest (the checkpoint is rebuilt from it with
seeded values by `sovits_checkpoint_weights`), its hot keys, and for every `dec.*` weight the reference folds (weight_g /
weight_v -> weight) the scale g / |v| it multiplied v by (v * scale equals the reference's tensor bit for bit); the md5
tables and the reference's md5 of seeded byte strings."""
import json
import os

import numpy as np
import pytest
import torch

from gsv_tts_lite_amd import loader, synth  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# upstream (RVC-Boss/GPT-SoVITS AR model) parameter names of one decoder layer, in the order of the lite names below
UPSTREAM_LAYER = ["self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
                  "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias",
                  "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias"]
LITE_LAYER = ["qkv.weight", "qkv.bias", "out_proj.weight", "out_proj.bias", "mlp.0.weight", "mlp.0.bias", "mlp.2.weight",
              "mlp.2.bias", "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias"]
SOVITS_CASES = [("v2Pro", b"05"), ("v2", b"01"), ("v2ProPlus", b"PK")]


def gpt_upstream_checkpoint():
    """(config, weights with upstream key names) of a 3-layer GPT on seeded weights"""
    cfg = synth.gpt_config(n_layer=3)
    w = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.gpt_weights(cfg, seed=9).items()}
    up = {}
    for l in range(3):
        for u, s in zip(UPSTREAM_LAYER, LITE_LAYER):
            up["model.h.layers.%d.%s" % (l, u)] = w["t2s_transformer.blocks.%d.%s" % (l, s)]
    for k in w:
        if not k.startswith("t2s_transformer."):
            up["model." + k] = w[k]
    return cfg, up


def sovits_checkpoint_weights(manifest):
    """the SoVITS checkpoint's weights from the reference module's state-dict manifest [[key, shape], ...]: seeded values,
    weight_g positive and independent of |weight_v| so that the fold is observable"""
    sd = {}
    for k, shape in manifest:
        a = synth.hashed_uniform("loader." + k, tuple(shape), 3)
        if k.endswith("weight_g"):
            a = np.abs(a) + np.float32(0.5)
        sd[k] = torch.from_numpy(a)
    return sd


def sovits_checkpoint(path, version, head, manifest):
    """write the .pth as upstream does ({"config", "weight"} pickle), its first two bytes replaced by `head`; -> the weights"""
    hps = synth.sovits_hps(version)
    if head != b"PK":
        hps["model"].pop("version", None)      # the 2-byte tag must supply it
    sd = sovits_checkpoint_weights(manifest)
    torch.save({"config": hps, "weight": sd}, str(path))
    raw = path.read_bytes()
    assert raw[:2] == b"PK"
    path.write_bytes(head + raw[2:])
    return sd


def md5_probe_bytes(n):
    """n seeded bytes (the reference hashed the same strings)"""
    return ((synth.hashed_uniform("loader.md5", (n,), 3) + 1.0) * 127.5).astype(np.uint8).tobytes()


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "loader.json")) as f:
        g = json.load(f)
    with np.load(os.path.join(GOLDEN, "loader.npz")) as z:
        g["fold_scale"] = {k: z[k] for k in z.files}
    return g


def test_gpt_ckpt_reference_loader_vs_product_loader(tmp_path, golden):
    G = golden["gpt"]
    cfg, up = gpt_upstream_checkpoint()
    path = tmp_path / "s1.ckpt"
    torch.save({"config": cfg, "weight": up}, str(path))
    config, mine = loader.read_gpt_checkpoint(str(path))
    assert config == G["config"]
    assert set(mine) == set(G["state"]), set(mine) ^ set(G["state"])
    for k, src in G["state"].items():
        assert torch.equal(up[src], mine[k]), k
    # and the safetensors directory the reference's TTS.to_safetensors layout names: the reference reads config.json and
    # loads model.safetensors into its module with safetensors' load_model (strict: exactly the module's keys)
    from safetensors.torch import load_file
    out = loader.convert_to_safetensors(str(path), str(tmp_path / "s1_dir"))
    with open(os.path.join(out, "config.json")) as f:
        assert json.load(f) == G["config"]
    st = load_file(os.path.join(out, "model.safetensors"))
    assert set(st) == set(G["state"]), set(st) ^ set(G["state"])
    for k, src in G["state"].items():
        assert torch.equal(st[k].float(), up[src]), k
        assert torch.equal(st[k].float(), mine[k]), k


@pytest.mark.parametrize("version,head", SOVITS_CASES)
def test_sovits_pth_reference_loader_vs_product_loader(tmp_path, golden, version, head):
    G = golden["sovits"][version]
    path = tmp_path / "s2.pth"
    sd = sovits_checkpoint(path, version, head, G["manifest"])
    assert any(k.startswith("dec.") and k.endswith("weight_g") for k in sd), "the Generator must arrive weight-normed"
    mine_hps, mine = loader.read_sovits_checkpoint(str(path))
    assert mine_hps["model"]["version"] == G["version"] == version
    hot = G["hot"]
    assert len(hot) > 100
    folded = {k for k in hot if k not in sd}
    assert folded == set(G["folded"]), folded ^ set(G["folded"])
    for k in hot:
        assert k in mine, k
        if k in folded:      # the reference's remove_weight_norm: weight = v * (g / |v|)
            ref = sd[k + "_v"] * torch.from_numpy(golden["fold_scale"][version + "/" + k])
        else:                # everything else the reference's load_state_dict took over unchanged
            ref = sd[k]
        np.testing.assert_allclose(mine[k].float().numpy(), ref.float().numpy(), rtol=2e-6, atol=1e-7, err_msg=k)
    assert not any(k.startswith("dec.") and k.endswith(("weight_g", "weight_v")) for k in mine)


def test_pretrained_md5_table_is_the_references(golden):
    assert loader.HASH_PRETRAINED == golden["hash_pretrained"]
    assert {k.decode(): v for k, v in loader.HEAD2VERSION.items()} == golden["head2version"]


def test_md5_version_lookup_on_a_pk_file(tmp_path, monkeypatch, golden):
    """a b"PK" file whose first 8 KiB hash is in the table gets its version from the table, as Loader.py:47-49"""
    for n, h_ref in golden["md5_probes"].items():     # the reference's hash of seeded files, shorter and longer than 8 KiB
        p = tmp_path / ("probe_%s" % n)
        p.write_bytes(md5_probe_bytes(int(n)))
        assert loader.get_hash_from_file(str(p)) == h_ref, n
    hps = synth.sovits_hps("v2Pro")
    hps["model"].pop("version", None)
    path = tmp_path / "s2G.pth"
    torch.save({"config": hps, "weight": {}}, str(path))
    h = loader.get_hash_from_file(str(path))
    monkeypatch.setitem(loader.HASH_PRETRAINED, h, "v2ProPlus")
    _, version = loader.read_sovits_file(str(path))
    assert version == "v2ProPlus"
