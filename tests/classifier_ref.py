"""CPU restatement of the four classifier heads of clip_dplm_amd/classifier.py as functions of a state dict, in plain
torch ops (eval mode: no dropout).  Checked against tests/golden/classifiers.npz - the reference classes' own logits, loss
and parameter gradients - by tests/test_classifier_host.py; the GPU tests compare the HIP modules to the same fixture.

TransformerClassifier: sequence length 1 (the reference feeds x.unsqueeze(0) to batch-second layers), so the softmax
weight of every row is exactly 1 and the attention block is out_proj(v_proj(x)); q and k never enter the value and their
rows of in_proj_weight / in_proj_bias get exact zero gradients."""
import torch
import torch.nn.functional as F


def mlp(sd, x):
    idx = sorted({int(k.split(".")[1]) for k in sd if k.startswith("mlp.")})
    for n, i in enumerate(idx):
        x = F.linear(x, sd[f"mlp.{i}.weight"], sd[f"mlp.{i}.bias"])
        if n < len(idx) - 1:
            x = F.relu(x)
    return x


def transformer(sd, x, eps=1e-5):
    h = F.linear(x, sd["input_projection.weight"], sd["input_projection.bias"])
    E = h.shape[1]
    n_layers = len({k.split(".")[2] for k in sd if k.startswith("transformer_encoder.layers.")})
    for i in range(n_layers):
        p = f"transformer_encoder.layers.{i}."
        v = F.linear(h, sd[p + "self_attn.in_proj_weight"][2 * E:], sd[p + "self_attn.in_proj_bias"][2 * E:])
        sa = F.linear(v, sd[p + "self_attn.out_proj.weight"], sd[p + "self_attn.out_proj.bias"])
        h = F.layer_norm(h + sa, (E,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], eps)
        ff = F.linear(F.relu(F.linear(h, sd[p + "linear1.weight"], sd[p + "linear1.bias"])), sd[p + "linear2.weight"],
                      sd[p + "linear2.bias"])
        h = F.layer_norm(h + ff, (E,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps)
    return F.linear(h, sd["output_projection.weight"], sd["output_projection.bias"])


def linear(sd, x):
    return F.linear(x, sd["linear.weight"], sd["linear.bias"])


def simple(sd, x, eps=1e-5):
    h = F.relu(F.linear(x, sd["layer1.weight"], sd["layer1.bias"]))
    h = F.layer_norm(h, (h.shape[1],), sd["norm.weight"], sd["norm.bias"], eps)
    return F.linear(h, sd["layer2.weight"], sd["layer2.bias"])


HEADS = {"mlp": mlp, "transformer": transformer, "linear": linear, "simple": simple}


def load_fixture(golden_dir):
    """{tag: dict(keys, sd, grads, logits, loss)}, x, labels from tests/golden/classifiers*.npz."""
    import os

    import numpy as np
    z = np.load(os.path.join(golden_dir, "classifiers.npz"))
    zt = np.load(os.path.join(golden_dir, "classifiers_transformer_grads.npz"))
    out = {}
    for tag in HEADS:
        keys = [str(k) for k in z[f"{tag}.keys"]]
        src = zt if tag == "transformer" else z
        out[tag] = dict(keys=keys, sd={k: torch.from_numpy(z[f"{tag}.w.{k}"]) for k in keys},
                        grads={k: torch.from_numpy(src[f"{tag}.g.{k}"]) for k in keys},
                        logits=torch.from_numpy(z[f"{tag}.logits"]), loss=float(z[f"{tag}.loss"]))
    return out, torch.from_numpy(z["x"]), torch.from_numpy(z["labels"])
