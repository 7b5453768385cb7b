"""Feature extraction for the reference's linear-probe baseline (lpclip/feat_extractor.py:113-137): the raw ``clip_model.visual(image)``
features of every image of a split, saved in the file ``lpclip/linear_probe.py`` reads.  The probe itself (sklearn) is not part of this
package."""
from __future__ import annotations

import os

import numpy as np
import torch


@torch.no_grad()
def extract_features(model, loader):
    """feat_extractor.py:118-129: ``model.encode_image`` (a ``zsclip.FrozenCLIP``) over the batches of ``loader`` (dicts with "img" and
    "label").  Returns (features float32 [N, embed_dim], labels int64 [N]) on the host, in loader order."""
    features, labels = [], []
    for batch in loader:
        features.append(model.encode_image(batch["img"]).cpu().to(torch.float32))
        labels.append(torch.as_tensor(batch["label"]).cpu().to(torch.int64).reshape(-1))
    if not features:
        return torch.zeros(0, model.shape.embed_dim, dtype=torch.float32), torch.zeros(0, dtype=torch.int64)
    return torch.cat(features), torch.cat(labels)


def save_features(output_dir, dataset_name, split, features, labels) -> str:
    """feat_extractor.py:130-137: ``{output_dir}/{dataset_name}/{split}.npz`` with the keys ``feature_list`` and ``label_list``."""
    save_dir = os.path.join(output_dir, dataset_name)
    os.makedirs(save_dir, exist_ok=True)
    path = os.path.join(save_dir, f"{split}.npz")
    np.savez(path, feature_list=np.asarray(torch.as_tensor(features).cpu(), dtype=np.float32),
             label_list=np.asarray(torch.as_tensor(labels).cpu(), dtype=np.int64))
    return path
