"""The classifier-probe loop of the reference's old/ablation.py: train a head on the frozen, concatenated embeddings of a
pre-trained CLIP model and report its accuracy.  train_classifier / evaluate take the reference's signatures
(old/ablation.py:20-49); batches are (a, b, labels).

Deviation, on purpose: the reference runs the frozen eval-mode CLIP model on every batch of every epoch
(ablation.py:27-28, :43).  Eval mode is deterministic, so the embeddings of a batch never change; `extract_embeddings`
computes them once per loader and train_classifier / evaluate iterate over the cached (a_embeds, b_embeds, labels)
embeddings - the same values, one CLIP forward per sample instead of one per sample and epoch; a shuffling loader's
per-epoch re-draw of the batches is kept (rows of the cache are re-drawn).  The two embedding tensors are
never concatenated for LinearClassifier (its fused loss reads both sources in place).
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import torch

from . import functional as KF
from .classifier import LinearClassifier, MLPClassifier, SimpleNonLinearClassifier, TransformerClassifier


def _embeds(outputs) -> Tuple[torch.Tensor, torch.Tensor]:
    """(a_embeds, b_embeds) of a CLIP module's output dict (old/clip.py:66-73: '<a>_embeds', '<b>_embeds' in that order)."""
    keys = [k for k in outputs if k.endswith("_embeds")]
    if len(keys) != 2:
        raise ValueError(f"expected two '*_embeds' entries in the CLIP outputs, got {list(outputs)}")
    return outputs[keys[0]], outputs[keys[1]]


@torch.no_grad()
def extract_embeddings(clip_model, loader, device=None) -> List[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]]:
    """[(a_embeds, b_embeds, labels)] per batch of `loader`, from ONE pass of the frozen eval-mode CLIP model (the module
    docstring has the deviation from the reference's per-epoch recomputation)."""
    was_training = clip_model.training
    clip_model.eval()
    dev = device if device is not None else next(clip_model.parameters()).device
    out = []
    for a, b, labels in loader:
        ea, eb = _embeds(clip_model(a.to(dev), b.to(dev)))
        out.append((ea.detach().float().contiguous(), eb.detach().float().contiguous(), labels.to(dev)))
    clip_model.train(was_training)
    return out


def train_clip(clip_model, train_loader, optimizer, num_epochs, device):
    """old/ablation.py:9-18: one-sided cross-entropy of the similarity logits against the diagonal."""
    clip_model.train()
    for _ in range(num_epochs):
        for a, b, _labels in train_loader:
            optimizer.zero_grad()
            outputs = clip_model(a.to(device), b.to(device))
            logits = next(v for k, v in outputs.items() if k.startswith("logits_per_"))
            loss = KF.cross_entropy_diag(logits, symmetric=False)
            loss.backward()
            optimizer.step()


def _shuffles(loader) -> bool:
    from torch.utils.data import RandomSampler
    return isinstance(getattr(loader, "sampler", None), RandomSampler)


def train_classifier(clip_model, classifier, train_loader, optimizer, num_epochs, device):
    """old/ablation.py:20-33.  optimizer: FusedAdamW(classifier, lr, weight_decay=0, max_grad_norm=None) is the
    reference's Adam; any torch optimiser works.  The embeddings of the whole dataset are cached once.  When the loader
    shuffles (DataLoader(..., shuffle=True) re-draws its batches every epoch, ablation.py:74) every epoch cuts the cached
    rows into batches of the loader's batch size in a new random order; otherwise the loader's own batches are revisited
    in its order.  Returns the last step's loss as a device tensor (no host sync here), None if no step ran."""
    batches = extract_embeddings(clip_model, train_loader, device)
    classifier.train()
    shuffle = _shuffles(train_loader) and len(batches) > 0
    if shuffle:
        ea, eb, labels = (torch.cat([b[i] for b in batches]) for i in range(3))
        n, bs = labels.shape[0], batches[0][2].shape[0]          # (a DataLoader's first batch is a full one)
    loss = None
    for _ in range(num_epochs):
        if shuffle:
            order = torch.randperm(n).to(labels.device)
            epoch = ((ea[idx], eb[idx], labels[idx]) for idx in order.split(bs))
        else:
            epoch = batches                                       # the loader's own batches, in its order
        for a, b, y in epoch:
            optimizer.zero_grad()
            loss = classifier.loss(a, y, x2=b)
            loss.backward()
            optimizer.step()
    return None if loss is None else loss.detach()


def evaluate(clip_model, classifier, test_loader, device):
    """old/ablation.py:35-49: accuracy.  The correct rows are counted on the device from the fused kernel's `pred`; one
    number is read at the end."""
    batches = extract_embeddings(clip_model, test_loader, device)
    classifier.eval()
    correct = torch.zeros((), dtype=torch.int64, device=device)
    total = 0
    for ea, eb, labels in batches:
        correct += (classifier.predict(ea, x2=eb) == labels).sum()
        total += labels.shape[0]
    return correct.item() / total


def ablation_study(config, rna_data, protein_data, diffmap_data, labels, num_classes, device, num_epochs=10,
                   batch_size=32, lr=1e-4) -> Dict[str, float]:
    """old/ablation.py:51-83: two CLIP models x four heads, accuracy on the training set (the reference's own protocol)."""
    from torch.utils.data import DataLoader, TensorDataset

    from .modeling_clip import DiffMapProteinCLIP, RNAProteinCLIP
    from .optim import FusedAdamW

    clip_models = {"RNA-Protein CLIP": RNAProteinCLIP(config).to(device),
                   "DiffMap-Protein CLIP": DiffMapProteinCLIP(config).to(device)}
    d = config.projection_dim * 2
    classifiers = {"MLP": MLPClassifier(d, [256, 128], num_classes).to(device),
                   "Transformer": TransformerClassifier(d, 256, num_classes, num_layers=2, num_heads=8).to(device),
                   "Linear": LinearClassifier(d, num_classes).to(device),
                   "SimpleNonLinear": SimpleNonLinearClassifier(d, 256, num_classes).to(device)}
    results = {}
    for clip_name, clip_model in clip_models.items():
        first = rna_data if clip_name == "RNA-Protein CLIP" else diffmap_data
        train_data = TensorDataset(first, protein_data, labels)
        train_loader = DataLoader(train_data, batch_size=batch_size, shuffle=True)
        train_clip(clip_model, train_loader, torch.optim.Adam(clip_model.parameters(), lr=lr), num_epochs, device)
        for clf_name, classifier in classifiers.items():
            opt = FusedAdamW(classifier, lr=lr, weight_decay=0.0, max_grad_norm=None)
            train_classifier(clip_model, classifier, train_loader, opt, num_epochs, device)
            results[f"{clip_name} + {clf_name}"] = evaluate(clip_model, classifier, DataLoader(train_data, batch_size=batch_size),
                                                            device)
    return results
