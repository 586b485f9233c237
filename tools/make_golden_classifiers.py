#!/usr/bin/env python
"""Write tests/golden/classifiers.npz (+ classifiers_transformer_grads.npz): the four classifier heads of the reference's
old/classifier.py, run on CPU in f32 and eval mode - state_dict key lists, weights, one input [37, 256], labels for 7
classes, logits, the nn.CrossEntropyLoss value and every parameter gradient.  Data only; the reference classes are
imported at run time from a checkout given on the command line:

    python tools/make_golden_classifiers.py --reference /path/to/clip-dplm

The TransformerClassifier's parameter gradients (its 2048-wide FFN) go to a second file so that each stays under 1 MiB.
"""
import argparse
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADS = {
    "mlp": ("MLPClassifier", (256, [64, 32], 7), {}),
    "transformer": ("TransformerClassifier", (256, 32, 7), {"num_layers": 1, "num_heads": 4}),
    "linear": ("LinearClassifier", (256, 7), {}),
    "simple": ("SimpleNonLinearClassifier", (256, 64, 7), {}),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference repository (holds old/classifier.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("ref_classifier", os.path.join(args.reference, "old", "classifier.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    torch.manual_seed(20240607)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(37, 256, generator=g)
    labels = torch.randint(0, 7, (37,), generator=g)
    main_file, tgrads = {"x": x.numpy(), "labels": labels.numpy()}, {}
    for tag, (cls, a, kw) in HEADS.items():
        m = getattr(ref, cls)(*a, **kw).eval()
        logits = m(x)
        loss = torch.nn.CrossEntropyLoss()(logits, labels)
        loss.backward()
        keys = list(m.state_dict().keys())
        main_file[f"{tag}.keys"] = np.array(keys)
        main_file[f"{tag}.logits"] = logits.detach().numpy()
        main_file[f"{tag}.loss"] = loss.detach().numpy()
        params = dict(m.named_parameters())
        for k, v in m.state_dict().items():
            main_file[f"{tag}.w.{k}"] = v.detach().numpy()
            (tgrads if tag == "transformer" else main_file)[f"{tag}.g.{k}"] = params[k].grad.numpy()
    np.savez_compressed(os.path.join(args.out, "classifiers.npz"), **main_file)
    np.savez_compressed(os.path.join(args.out, "classifiers_transformer_grads.npz"), **tgrads)
    for f in ("classifiers.npz", "classifiers_transformer_grads.npz"):
        print(f, os.path.getsize(os.path.join(args.out, f)), "bytes")


if __name__ == "__main__":
    main()
