"""The timing loop of the loss benchmarks (scripts/bench_{lpips,lpips_alex,vgg_loss,parse_loss,id_loss}.py): every case under the HIP path
(`module.fused = True`) and the ATen path of the same module (`fused = False`), alternated in one process."""
import statistics

PATHS = {'hip': True, 'aten': False}


def measure(module, cases, blocks, iters, warmup, hip_call=None, launches=False):
    """cases: {name: callable()}; every callable is run under both paths of `module` (its `fused` switch is left at the last one: the caller
    restores it) -> {name: {path: figures}}: the device-event median over `blocks` alternating blocks of the time per call, the spread of
    the blocks (max - min), the block times, the peak memory of one call (torch.cuda.max_memory_allocated minus what was allocated before
    it) and, with `launches`, the library launches of one call by entry point.  `hip_call`: an entry point that only the module's HIP path
    launches; the warm-up then asserts that each path took the route its switch names."""
    import torch
    from torch_utils import hip_plugin
    for name, fn in cases.items():
        for fused in PATHS.values():
            module.fused = fused
            before = hip_plugin.CALLS.get(hip_call, 0)
            for _ in range(warmup):
                fn()
            if hip_call is not None:
                took_hip = hip_plugin.CALLS.get(hip_call, 0) > before
                assert took_hip == fused, f'{name}: fused = {fused} but the HIP loss head ' + ('ran' if took_hip else 'did not run')
    torch.cuda.synchronize()
    times = {(c, p): [] for c in cases for p in PATHS}
    for _ in range(blocks):
        for c, fn in cases.items():
            for p, fused in PATHS.items():
                module.fused = fused
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[(c, p)].append(e0.elapsed_time(e1) / iters)
    out = {}
    for c, fn in cases.items():
        out[c] = {}
        for p, fused in PATHS.items():
            module.fused = fused
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            before = dict(hip_plugin.CALLS)
            fn()
            torch.cuda.synchronize()
            t = times[(c, p)]
            out[c][p] = dict(ms=round(statistics.median(t), 3), spread_ms=round(max(t) - min(t), 3), blocks_ms=[round(v, 3) for v in t],
                             peak_mib=round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1))
            if launches:
                out[c][p]['launches'] = {k: v - before.get(k, 0) for k, v in hip_plugin.CALLS.items() if v != before.get(k, 0)}
        out[c]['hip_over_aten'] = round(out[c]['hip']['ms'] / out[c]['aten']['ms'], 3)
    return out
