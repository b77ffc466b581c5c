#!/usr/bin/env python3
"""tests/golden/id_loss.npz: the ArcFace identity loss and its image gradient from the REFERENCE's own classes.

`inversion.psp.encoders.model_irse.Backbone(112, 50, mode='ir_se', drop_ratio=0.6)` and `inversion.criteria.id_loss.IDLoss` are imported at
run time (oracle/ref_import.py).  The backbone gets `tests/id_loss_ref.py::synthetic_state_dict` weights (a function of the parameter
names); the loss object is created without running its constructor, which loads a weights file: `__new__`, `nn.Module.__init__`, then its
attributes set by hand.  Its own `extract_feats` and `forward` run on the CPU.  Per case: the two images as uint8 (value = u8 / 127.5 - 1),
both embeddings, the loss, `sim_improvement`, and of the image gradient every 4th row and column inside the crop with its float64 sum and
L2 norm (it is zero outside the crop).  Also the state-dict key list.

    python scripts/make_id_loss_golden.py          (needs the reference tree, see oracle/ref_import.py)
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
    import id_loss_ref as R
    from inversion.criteria.id_loss import IDLoss
    from inversion.psp.encoders.model_irse import Backbone
    torch.manual_seed(5)
    net = Backbone(112, 50, mode='ir_se', drop_ratio=0.6)
    net.load_state_dict(R.synthetic_state_dict({k: list(v.shape) for k, v in net.state_dict().items()}))
    net.eval().requires_grad_(False)
    crit = IDLoss.__new__(IDLoss)
    torch.nn.Module.__init__(crit)
    crit.facenet, crit.pool, crit.face_pool = net, torch.nn.AdaptiveAvgPool2d((256, 256)), torch.nn.AdaptiveAvgPool2d((112, 112))
    out = {'keys': np.array(list(net.state_dict().keys()))}
    stds = []
    hooks = [m.register_forward_hook(lambda _m, _i, o: stds.append(float(o.detach().std()))) for m in [net.input_layer, *net.body]]
    for i, shape in enumerate(R.CASES):
        y_hat, y = R.smooth_images(shape, 11 + i), R.smooth_images(shape, 21 + i)
        leaf = R.to_float(y_hat).requires_grad_(True)
        yt = R.to_float(y)
        del stds[:]
        loss, sim, logs = crit(leaf, yt, yt)
        spread = stds[-len(net.body) - 1:]
        (grad,) = torch.autograd.grad(loss, [leaf])
        with torch.no_grad():
            out[f'{i}/feats_hat'], out[f'{i}/feats'] = crit.extract_feats(leaf.detach()).numpy(), crit.extract_feats(yt).numpy()
        f = shape[2] // 256
        outside = grad.clone()
        outside[:, :, 35 * f:223 * f, 32 * f:220 * f] = 0
        assert float(outside.abs().max()) == 0.0
        out[f'{i}/y_hat'], out[f'{i}/y'] = y_hat, y
        out[f'{i}/loss'], out[f'{i}/sim_improvement'] = np.float32(loss.detach().numpy()), np.float64(sim)
        out[f'{i}/grad_samples'] = R.crop_samples(grad).contiguous().numpy()
        out[f'{i}/grad_sum'], out[f'{i}/grad_norm'] = np.float64(grad.double().sum()), np.float64(grad.double().norm())
        # how far ATen's fp32 CPU run is from float64 on this case (what a tolerance against the fixture rests on)
        l64, g64, _, _ = R.loss64(net, R.to_float(y_hat), yt, R.IR_SE50['units'])
        print(f'case {i} {shape}: loss {float(loss):.6f} (float64 {l64:.6f}, diff {abs(float(loss) - l64):.2e}), sim {sim:.4f}, '
              f'|grad| {float(grad.norm()):.4e}, max |grad - float64| / max |grad| {float((grad.double() - g64).abs().max() / g64.abs().max()):.2e}; '
              f'activation std: input layer {spread[0]:.2f}, blocks {min(spread[1:]):.2f}..{max(spread[1:]):.2f}')
    for h in hooks:
        h.remove()
    path = os.path.join(ROOT, 'tests', 'golden', 'id_loss.npz')
    np.savez_compressed(path, **out)
    print(f'wrote {path} ({os.path.getsize(path) / 1024:.0f} KB)')


if __name__ == '__main__':
    main()
