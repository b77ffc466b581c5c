"""The CLIP image-text loss (training/clip_loss.py) without a GPU: the image tower's keys and shapes, the preprocessing against the
reference's two torch modules, the PyTorch definition against a float64 functional restatement (tests/clip_loss_ref.py) and against the
independent implementation in `transformers`, the orchestration of the fused pass - run here on a float64 torch restatement of every launch
(`TorchOps`) - against float64 autograd, the head's closed-form gradient, the closure for the projector and the routing rules."""

import pytest
import torch
import torch.nn as nn

import clip_loss_ref as R


def _expected_keys(width=768, layers=12, patch=32, tokens=50, dim=512):
    C = width
    keys = {'class_embedding': (C,), 'positional_embedding': (tokens, C), 'proj': (C, dim), 'conv1.weight': (C, 3, patch, patch),
            'ln_pre.weight': (C,), 'ln_pre.bias': (C,), 'ln_post.weight': (C,), 'ln_post.bias': (C,)}
    for i in range(layers):
        b = f'transformer.resblocks.{i}.'
        keys.update({b + 'ln_1.weight': (C,), b + 'ln_1.bias': (C,), b + 'attn.in_proj_weight': (3 * C, C), b + 'attn.in_proj_bias': (3 * C,),
                     b + 'attn.out_proj.weight': (C, C), b + 'attn.out_proj.bias': (C,), b + 'ln_2.weight': (C,), b + 'ln_2.bias': (C,),
                     b + 'mlp.c_fc.weight': (4 * C, C), b + 'mlp.c_fc.bias': (4 * C,), b + 'mlp.c_proj.weight': (C, 4 * C), b + 'mlp.c_proj.bias': (C,)})
    return keys


def test_state_dict_keys_and_shapes_are_clips_visual_module():
    from training import clip_loss
    with torch.device('meta'):
        net = clip_loss.VisionTransformer()
    got = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert got == _expected_keys() and len(got) == 8 + 12 * 12
    assert sum(v.numel() for v in net.state_dict().values()) * 4 == 351_396_864          # the 351 MB the documents quote
    assert 'RANDOMLY INITIALISED' in clip_loss.CLIPLoss.__doc__ and 'RANDOMLY INITIALISED' in clip_loss.__doc__
    assert 'tokenizer' in clip_loss.__doc__.lower() and 'tokenizer' in clip_loss.CLIPLoss.__doc__.lower()


def test_load_clip_state_dict_takes_the_prefix_and_fp16_values():
    from training import clip_loss
    src = R.visual(R.ODD)
    sd = src.state_dict()
    full = {'visual.' + k: v.half() for k, v in sd.items()}
    full.update({'token_embedding.weight': torch.zeros(4, 4), 'logit_scale': torch.zeros([])})
    a = clip_loss.VisionTransformer(**R.ODD).load_clip_state_dict(full)
    b = clip_loss.VisionTransformer(**R.ODD).load_clip_state_dict(sd)
    for k, v in sd.items():
        assert a.state_dict()[k].dtype == torch.float32 and torch.equal(a.state_dict()[k], v.half().float()) and torch.equal(b.state_dict()[k], v), k
    with pytest.raises(RuntimeError):
        clip_loss.VisionTransformer(**R.ODD).load_clip_state_dict({k: v for k, v in sd.items() if k != 'proj'})
    crit = clip_loss.CLIPLoss(stylegan_size=64, visual=clip_loss.VisionTransformer(**R.ODD), weights=full)
    assert torch.equal(crit.visual.proj, sd['proj'].half().float()) and not crit.visual.training and not any(p.requires_grad for p in crit.parameters())
    crit.train()
    assert not crit.visual.training
    c = clip_loss.VisionTransformer.from_clip_state_dict({'visual.' + k: v for k, v in R.visual(R.NARROW).state_dict().items()})
    assert (c.width, c.layers, c.patch_size, c.tokens, c.output_dim, c.input_resolution) == (64, 12, 32, 50, 32, 224)


@pytest.mark.parametrize('S', [32, 64, 96, 224, 512])
def test_preprocess_equals_the_two_torch_modules(S):
    crit = R.cliploss(R.ODD, S)
    x = R.images((2, 3, S, S), S)
    want = nn.AvgPool2d(kernel_size=S // 32)(nn.Upsample(scale_factor=7)(x))
    got = crit.preprocess(x)
    assert tuple(got.shape) == (2, 3, 224, 224) and torch.equal(got, want)
    if S == 224:
        assert float((got - x).abs().max()) <= 48 * 2 ** -24, 'k = 7: the identity, up to the 48 roundings of ATen\'s fp32 sum of 49 equal values (|x| <= 1)'
    norm = R.cliploss(R.ODD, S, normalise=True).preprocess(x)
    m, s = (torch.tensor(v).reshape(1, 3, 1, 1) for v in (R.CLIP_MEAN, R.CLIP_STD))
    assert torch.equal(norm, ((want + 1) / 2 - m) / s)


@pytest.mark.parametrize('spec,S', [('NARROW', 64), ('ODD', 96), ('B16', 64)])
def test_definition_equals_the_float64_restatement(spec, S):
    """Both in float64: they differ by rounding order only (1e-10 of the largest magnitude; a wrong scale, order of heads or a dropped
    bias is 1e-2 or more)."""
    crit = R.cliploss(getattr(R, spec), S, dtype=torch.float64, normalise=(spec == 'ODD'))
    x, text = R.images((2, 3, S, S), 1).double(), R.rows((3, crit.visual.output_dim), 2).double()
    kw = dict(mean=crit.mean, std=crit.std)
    l64, g64, out64, f64 = R.loss64(crit.visual, x, text, **kw)
    f = crit.features(x)
    assert crit.last_path == 'torch' and float((f - f64).abs().max()) <= 1e-10 * float(f64.abs().max())
    leaf = x.clone().requires_grad_(True)
    out = crit(leaf, text)
    assert tuple(out.shape) == (2, 3) and float((out.detach() - out64).abs().max()) <= 1e-10
    (g,) = torch.autograd.grad(crit.distance_to(leaf, text), [leaf])
    assert abs(float(out.detach().mean()) - l64) <= 1e-10 and float((g - g64).abs().max()) <= 1e-10 * float(g64.abs().max())
    # the directional loss against the restatement
    base, direction = R.rows((2, crit.visual.output_dim), 3).double(), R.rows((crit.visual.output_dim,), 4).double()
    d64, dg64, _, _ = R.loss64(crit.visual, x, direction, base, **kw)
    leaf = x.clone().requires_grad_(True)
    d = crit.directional(leaf, base, direction)
    (dg,) = torch.autograd.grad(d, [leaf])
    assert abs(float(d.detach()) - d64) <= 1e-10 and float((dg - dg64).abs().max()) <= 1e-10 * float(dg64.abs().max())


def test_embeddings_equal_the_transformers_implementation():
    """An independent implementation of the same tower (random, built offline), weights copied under the key map of the two code bases."""
    tr = pytest.importorskip('transformers')
    spec = dict(width=64, heads=2, layers=3, patch_size=32, output_dim=32)
    net = R.visual(spec).double()
    cfg = tr.CLIPVisionConfig(hidden_size=64, intermediate_size=256, num_hidden_layers=3, num_attention_heads=2, image_size=224, patch_size=32,
                              projection_dim=32, hidden_act='quick_gelu', layer_norm_eps=1e-5, attention_dropout=0.0)
    cfg._attn_implementation = 'sdpa'          # (the eager form rounds the probabilities to float32 whatever the dtype)
    other = tr.CLIPVisionModelWithProjection(cfg).double().eval()
    sd = net.state_dict()
    C = 64
    m = {'vision_model.embeddings.class_embedding': sd['class_embedding'], 'vision_model.embeddings.patch_embedding.weight': sd['conv1.weight'],
         'vision_model.embeddings.position_embedding.weight': sd['positional_embedding'],
         'vision_model.pre_layrnorm.weight': sd['ln_pre.weight'], 'vision_model.pre_layrnorm.bias': sd['ln_pre.bias'],
         'vision_model.post_layernorm.weight': sd['ln_post.weight'], 'vision_model.post_layernorm.bias': sd['ln_post.bias'],
         'visual_projection.weight': sd['proj'].t()}
    for i in range(3):
        a, b = f'transformer.resblocks.{i}.', f'vision_model.encoder.layers.{i}.'
        for j, name in enumerate(('q_proj', 'k_proj', 'v_proj')):
            m[b + f'self_attn.{name}.weight'] = sd[a + 'attn.in_proj_weight'][j * C:(j + 1) * C]
            m[b + f'self_attn.{name}.bias'] = sd[a + 'attn.in_proj_bias'][j * C:(j + 1) * C]
        for src, dst in (('attn.out_proj', 'self_attn.out_proj'), ('ln_1', 'layer_norm1'), ('ln_2', 'layer_norm2'), ('mlp.c_fc', 'mlp.fc1'), ('mlp.c_proj', 'mlp.fc2')):
            m[b + dst + '.weight'], m[b + dst + '.bias'] = sd[a + src + '.weight'], sd[a + src + '.bias']
    own = other.state_dict()
    extra = {k: own[k] for k in own if k not in m}
    assert all('position_ids' in k for k in extra), sorted(extra)
    other.load_state_dict({**{k: v.clone().contiguous() for k, v in m.items()}, **extra}, strict=True)
    x = R.images((2, 3, 224, 224), 6).double()
    with torch.no_grad():
        want = other(pixel_values=x).image_embeds
        got = net(x)
    assert tuple(got.shape) == (2, 32) and float((got - want).abs().max()) <= 1e-10 * float(want.abs().max())


@pytest.mark.parametrize('spec,shape,normalise', [('ODD', (2, 3, 96, 96), True), ('NARROW', (1, 3, 64, 64), False)])
def test_fused_orchestration_against_float64_autograd(spec, shape, normalise):
    """`_fused_forward` / `_fused_backward` - what the HIP path runs - with every launch restated in float64 torch: rows, embeddings and
    image gradient equal float64 autograd of the functional restatement to rounding (a dropped skip gradient, a wrong transposed weight or
    a mis-ordered patch channel is 1e-2 or more)."""
    from training import clip_loss
    crit = R.cliploss(getattr(R, spec), shape[2], dtype=torch.float64, normalise=normalise)
    net = crit.visual
    x = R.images(shape, 7).double()
    text, base = R.rows((3, net.output_dim), 8).double(), R.rows((shape[0], net.output_dim), 9).double()
    kw = dict(mean=crit.mean, std=crit.std)
    ops = R.TorchOps(torch.float64)
    dout = R.rows((shape[0], 3), 10).double()
    for b in (None, base):
        sd = {k: v.double() for k, v in net.state_dict().items()}
        leaf = x.clone().requires_grad_(True)
        f64 = R.embed(sd, leaf, net.heads, **kw)
        out64 = R.cosine_rows(f64, text, b)
        (g64,) = torch.autograd.grad((out64 * dout).sum(), [leaf])
        f64, out64 = f64.detach(), out64.detach()
        with torch.no_grad():
            out, avg, f, sv = clip_loss._fused_forward(ops, net, x, text, b, crit.mean, crit.std)
            grad = clip_loss._fused_backward(ops, net, sv, dout)
            assert clip_loss._fused_forward(ops, net, x, None, None, crit.mean, crit.std)[0] is None
        assert float((f - f64).abs().max()) <= 1e-10 * float(f64.abs().max())
        assert float((out - out64).abs().max()) <= 1e-10 and abs(float(avg - out64.mean())) <= 1e-10
        assert tuple(grad.shape) == shape and float((grad - g64).abs().max()) <= 1e-9 * float(g64.abs().max())


def test_the_heads_closed_form_gradient_as_the_fused_backward_uses_it():
    """`clip_loss._fused_backward` turns dout into the embeddings' gradient with the closed form df = (g - e (e . g)) / norm; its first two
    steps (head_backward, then the projection's input gradient) are run here on the float64 ops with a recording `linear_backward_input`,
    and what reaches it equals autograd through the head."""
    from training import clip_loss

    class Stop(Exception):
        pass

    class Ops(R.TorchOps):
        def linear_backward_input(self, dy, w):
            self.df = dy
            raise Stop

    net = R.visual(R.ODD).double()
    f, text, base, dout = R.rows((3, 20), 11).double(), R.rows((4, 20), 12).double() * 3, R.rows((3, 20), 13).double(), R.rows((3, 4), 14).double()
    for b in (None, base):
        ops = Ops(torch.float64)
        leaf = f.clone().requires_grad_(True)
        out, e, norm, tnorm, avg = ops.head(leaf, text, b)
        (want,) = torch.autograd.grad((out * dout).sum(), [leaf])
        sv = dict(e=e.detach(), text=text, norm=norm.detach(), tnorm=tnorm)
        with pytest.raises(Stop):
            clip_loss._fused_backward(ops, net, sv, dout)
        assert float((ops.df - want).abs().max()) <= 1e-12 * float(want.abs().max())
        assert float((out.detach() - R.cosine_rows(f, text, b)).abs().max()) <= 1e-14 and abs(float(avg.detach() - out.detach().mean())) <= 1e-15


def test_switches_and_cpu_routing():
    """Without a GPU everything takes the PyTorch definition; the host-side limits refuse what the fused route does not cover."""
    from training import clip_loss
    assert isinstance(clip_loss.fused, bool) and clip_loss.arith == 0
    crit = R.cliploss(R.ODD, 64)
    x, text = R.images((1, 3, 64, 64), 15), R.rows((2, 20), 16)
    assert not clip_loss._on_hip(crit.visual, x), 'CPU tensors'
    out = crit(x, text)
    assert crit.last_path == 'torch' and tuple(out.shape) == (1, 2)
    assert torch.equal(crit.distance_to(x, text), out.mean()) and torch.equal(crit(x, text[0]), out[:, :1])
    for spec in (R.NARROW, R.WIDE, R.ODD, dict(clip_loss_default=True)):
        with torch.device('meta'):
            net = clip_loss.VisionTransformer() if 'clip_loss_default' in spec else clip_loss.VisionTransformer(**spec)
        assert clip_loss._net_ok(net), spec
    bad = (R.B16,                                                                              # 65 tokens
           dict(width=768, heads=12, layers=1, patch_size=16, output_dim=512),                 # ViT-B/16: 197 tokens
           dict(width=136, heads=2, layers=1, patch_size=32, output_dim=32),                   # head dimension 68
           dict(width=60, heads=10, layers=1, patch_size=32, output_dim=32),                   # head dimension 6
           dict(width=64, heads=2, layers=1, patch_size=32, output_dim=30),                    # D no multiple of 4
           dict(width=64, heads=2, layers=1, patch_size=32, output_dim=32, input_resolution=256))
    for spec in bad:
        with torch.device('meta'):
            assert not clip_loss._net_ok(clip_loss.VisionTransformer(**spec)), spec
    # a trainable parameter: the definition, and its gradient exists
    p = crit.visual.ln_post.weight
    p.requires_grad_(True)
    try:
        crit.distance_to(x, text).backward()
        assert crit.last_path == 'torch' and p.grad is not None
    finally:
        p.requires_grad_(False)
        p.grad = None


def test_clip_distance_with_a_base_is_the_hand_written_sum():
    from training import clip_loss, projection
    crit = R.cliploss(R.ODD, 64)
    text = R.rows((2, 20), 17)
    images, other = ((R.images((1, 3, 64, 64), s) + 1) * 127.5 for s in (18, 19))
    base = projection.l2_distance(other)
    d = clip_loss.clip_distance(text, crit, weight=0.25, base=base)
    assert torch.equal(d(images), 0.25 * crit.distance_to(images / 127.5 - 1, text) + base(images))
    assert torch.equal(clip_loss.clip_distance(text, crit)(images), crit.distance_to(images / 127.5 - 1, text))
    leaf = images.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(d(leaf), [leaf])
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
