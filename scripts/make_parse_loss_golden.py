#!/usr/bin/env python3
"""tests/golden/parse_loss.npz: the face parser's cross-entropy loss and its image gradient from the REFERENCE's own BiSeNet.

The reference class (inversion/BiSeNet.py) is imported at run time (oracle/ref_import.py), given `oracle/face_parsing.py::synthetic_state_dict`
weights (a function of the parameter names) and run on the CPU with `torch.nn.CrossEntropyLoss()` and autograd, as the apps do
(apps/train_hybrid_encoder.py:279-283).  Per case: the image, the labels, the loss, the image gradient.

    python scripts/make_parse_loss_golden.py          (needs the reference tree, see oracle/ref_import.py)
"""

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_import  # noqa: E402

ref_import.install()

import numpy as np  # noqa: E402
import torch  # noqa: E402

CASES = (((2, 3, 64, 64), 101), ((1, 3, 96, 64), 102))          # (image shape, seed)


def inputs(shape, seed):
    """The image (uniform in -1..1) and the labels (uniform in 0..19) of a case."""
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(shape, generator=g) * 2 - 1
    lab = torch.randint(0, 20, (shape[0], shape[2], shape[3]), generator=g)
    return img, lab


def main():
    from inversion.BiSeNet import BiSeNet
    from oracle import face_parsing as ofp
    torch.manual_seed(5)
    net = BiSeNet(n_classes=20).eval()
    net.load_state_dict(ofp.synthetic_state_dict({k: list(v.shape) for k, v in net.state_dict().items()}))
    net.requires_grad_(False)
    out = {}
    for i, (shape, seed) in enumerate(CASES):
        img, lab = inputs(shape, seed)
        leaf = img.clone().requires_grad_(True)
        loss = torch.nn.CrossEntropyLoss()(net(leaf)[0], lab)
        (grad,) = torch.autograd.grad(loss, [leaf])
        out[f'{i}/image'], out[f'{i}/labels'] = img.numpy(), lab.numpy().astype(np.uint8)
        out[f'{i}/loss'], out[f'{i}/grad'] = loss.detach().numpy(), grad.numpy()
        print(f'case {i} {shape}: loss {float(loss):.6f}, |grad| {float(grad.norm()):.4e}')
    path = os.path.join(ROOT, 'tests', 'golden', 'parse_loss.npz')
    np.savez_compressed(path, **out)
    print(f'wrote {path} ({os.path.getsize(path) / 1024:.0f} KB)')


if __name__ == '__main__':
    main()
