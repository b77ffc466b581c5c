#!/usr/bin/env python3
"""tests/golden/discriminator.npz: logits and the generator loss's image gradient from the REFERENCE's own discriminator class.

`inversion.networks.Discriminator` is imported at run time (oracle/ref_import.py) in the tiny configuration
`tests/adv_loss_ref.py::CASES['fixture']`, gets `synthetic_state_dict` weights (a function of the parameter names and a seed) and runs on
the CPU.  Recorded: the state dict (`sd/<key>`, buffers included) and its key order, the inputs, the logits, and the image gradient of
`softplus(-logits).mean()`.  A recipe, not a test: it needs the reference tree and never runs where that is missing.

    python scripts/make_discriminator_golden.py
"""

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from oracle import ref_import  # noqa: E402

ref_import.install()

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    import adv_loss_ref as R
    from inversion.networks import Discriminator
    D = R.build('fixture', Discriminator)
    img, c = R.case_inputs('fixture')
    leaf = img.clone().requires_grad_(True)
    logits = D(leaf, c)
    loss = torch.nn.functional.softplus(-logits).mean()
    (grad,) = torch.autograd.grad(loss, [leaf])
    sd = D.state_dict()
    out = {'keys': np.array(list(sd.keys())), 'img': img.numpy(), 'c': c.numpy(), 'logits': logits.detach().numpy(), 'loss': np.float32(loss.item()),
           'grad': grad.numpy()}
    out.update({'sd/' + k: v for k, v in R.to_numpy_state(sd).items()})
    # how far the reference's fp32 CPU run is from the float64 restatement (what the parity test's tolerance rests on)
    taps = []
    l64, g64, z64 = R.loss64(sd, R.CASES['fixture']['kwargs'], img, c, taps=taps)
    print(f'{sum(p.numel() for p in D.parameters())} parameters; loss {float(loss):.7f} (float64 {l64:.7f}); logits rel {R.rel_l2(logits.detach()[:, 0], z64):.2e}, '
          f'gradient rel L2 {R.rel_l2(grad, g64):.2e}; kink margin {R.kink_margin(taps):.2e}')
    path = os.path.join(ROOT, 'tests', 'golden', 'discriminator.npz')
    np.savez_compressed(path, **out)
    print(f'wrote {path} ({os.path.getsize(path) / 1024:.0f} KB)')


if __name__ == '__main__':
    main()
