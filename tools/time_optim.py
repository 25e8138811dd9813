"""Times one optimizer step on the full model's real parameter list (the trainable parameters of MVXNet in train_like.py's
bucket layout), gradient = the SUM over the frames with the frame count in the bucket's count slot:
  * hip        -- modules/optim.py: norm + prepare + update launches, the division by the count folded into the update;
  * torch      -- the default path: ``flat.div_(count)`` + torch.optim.AdamW(fused=True).step();
  * hip_clip   -- the same call with max_norm set (the norm is computed either way);
  * torch_clip -- ``flat.div_`` + ``clip_grad_norm_(foreach=True)`` + the fused step.
The variants alternate inside one process; each run is --inner steps between two device events; medians (and minima) over
--rounds runs after --warmup.  Also reported: the achieved fraction of the measured copy rate (6.29 TB/s) for the 7 x 4 x N bytes
the update has to move (read p, g, m, v; write p, m, v) -- the whole working set fits the Infinity Cache, so this is a rate
against the HBM copy figure, not an HBM measurement.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'mvxnet-makise_amd'), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

COPY_RATE = 6.29e12          # bytes / s, the measured device copy rate


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--inner', type=int, default=20)
    args = ap.parse_args()
    if args.rounds < 20:
        raise SystemExit('--rounds: at least 20 alternating runs')
    sys.argv = sys.argv[:1]
    import torch
    import modules.config as cfg
    from modules import optim, parallel
    from MVXNet import MVXNet

    dev = torch.device('cuda')
    torch.manual_seed(0)

    def make():
        model = MVXNet().to(dev)
        params = [p for p in model.parameters() if p.requires_grad]
        bucket = parallel.GradBucket(params, late=[model.head.fusion.fcn1.fc.weight])
        return model, params, bucket

    _, p_hip, b_hip = make()
    _, p_tor, b_tor = make()
    g = torch.Generator(device=dev).manual_seed(1)
    grad = torch.randn(b_hip.flat.numel(), generator=g, device=dev) * 1e-2
    n = grad.numel()
    o_hip = optim.AdamW(p_hip, lr=1e-3, eps=cfg.eps, bucket=b_hip)
    o_tor = torch.optim.AdamW(p_tor, lr=1e-3, eps=cfg.eps, fused=True)
    tables = {'aligned_chunks': 0, 'scalar_chunks': 0}
    for addr, off, cnt in o_hip._table.cpu().tolist():
        ok = addr % 16 == 0 and (b_hip.flat.data_ptr() + 4 * off) % 16 == 0
        tables['aligned_chunks' if ok else 'scalar_chunks'] += 1

    def hip(max_norm):
        def run():
            o_hip.max_norm = max_norm
            for _ in range(args.inner):
                b_hip.flat.copy_(grad)
                b_hip.count_slot().fill_(4.0)
                o_hip.step(count=b_hip.count_slot())
        return run

    def tor(max_norm):
        def run():
            for _ in range(args.inner):
                b_tor.flat.copy_(grad)
                b_tor.count_slot().fill_(4.0)
                b_tor.flat.div_(b_tor.count_slot().clamp_min(1.0))
                if max_norm > 0:
                    torch.nn.utils.clip_grad_norm_(p_tor, max_norm, foreach=True)
                o_tor.step()
        return run

    def fill_only():
        for _ in range(args.inner):
            b_hip.flat.copy_(grad)
            b_hip.count_slot().fill_(4.0)

    variants = [('fill', fill_only), ('hip', hip(0.0)), ('torch', tor(0.0)), ('hip_clip', hip(1.0)), ('torch_clip', tor(1.0))]
    us = {name: [] for name, _ in variants}
    for k in range(args.warmup + args.rounds):
        for name, fn in variants:
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            if k >= args.warmup:
                us[name].append(s.elapsed_time(e) * 1e3 / args.inner)
    res = {'n': n, 'mbytes_per_tensor': round(4 * n / 1e6, 2), 'rounds': args.rounds, 'inner': args.inner, **tables}
    fill = statistics.median(us['fill'])
    res['fill_us'] = round(fill, 2)           # the gradient refill that every variant's step includes
    for name, _ in variants[1:]:
        med = statistics.median(us[name]) - fill
        res[name + '_us'] = round(med, 2)
        res[name + '_min_us'] = round(min(us[name]) - fill, 2)
        res[name + '_copy_rate_fraction'] = round(7 * 4 * n / (med * 1e-6) / COPY_RATE, 4)
    d = o_hip.diagnostics()
    assert d['skipped'] == 0 and d['step'] == (args.warmup + args.rounds) * args.inner * 2, d
    print(json.dumps(res))


if __name__ == '__main__':
    main()
