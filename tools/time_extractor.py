"""Times the frozen ResNet50-FPN image extractor (modules/imhead/Extractor.py) on 4 frames of 370 x 1224 u8 with the seeded
test weights, between device events, in ``bf16x6`` and ``f32``: preparation, stem convolution, max pool, the four body stages,
the FPN, and the whole chain.  Each piece runs on the true output of the piece before it.  Prints one JSON line (medians over
--iters calls after --warmup, in ms for the 4 frames) with the derived work of 77 GMAC per frame next to it."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'mvxnet-makise_amd'), os.path.join(ROOT, 'tests'), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def gmac_per_frame(ph=416, pw=1344):
    """Multiply-accumulates of one frame, by part, from the layer shapes."""
    from modules.imhead.Extractor import LAYERS
    h, w = ph // 4, pw // 4
    parts = {'stem': (ph // 2) * (pw // 2) * 64 * 147}
    cin, body = 64, 0
    for li, (n, width) in enumerate(LAYERS):
        for b in range(n):
            hin, win = h, w
            if b == 0 and li > 0:
                h, w = h // 2, w // 2
            body += hin * win * cin * width + h * w * width * width * 9 + h * w * width * 4 * width
            if b == 0:
                body += h * w * cin * 4 * width
            cin = 4 * width
    parts['body'] = body
    parts['fpn_lateral'] = sum((ph // s) * (pw // s) * c * 256 for s, c in ((4, 256), (8, 512), (16, 1024), (32, 2048)))
    parts['fpn_output'] = sum((ph // s) * (pw // s) * 256 * 256 * 9 for s in (4, 8, 16))
    parts['total'] = sum(parts.values())
    return {k: round(v / 1e9, 2) for k, v in parts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--frames', type=int, default=4)
    args = ap.parse_args()
    sys.argv = sys.argv[:1]
    import numpy as np
    import torch
    import modules.config as cfg
    from modules import _hip
    from modules.imhead.Pipe import ImageFeatureExtractor
    import extractor_ref as R

    dev = torch.device('cuda')
    ex = ImageFeatureExtractor().load_weights(R.f32_state_dict()).to(dev)
    net = ex._network(dev)
    img = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (args.frames, 370, 1224, 3), dtype=np.uint8)).to(dev)

    def timed(fn):
        ms = []
        for k in range(args.warmup + args.iters):
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            if k >= args.warmup:
                ms.append(s.elapsed_time(e))
        return round(statistics.median(ms), 3)

    res = {'frames': args.frames, 'iters': args.iters, 'gmac_per_frame': gmac_per_frame()}
    old = cfg.config.get('convmath', 'f32')
    try:
        for math in ('bf16x6', 'f32'):
            cfg.config['convmath'] = math
            with torch.no_grad():
                x4 = net.prepare(img)
                conv = _hip.stem_conv7(x4, net.stem_w, net.stem_b)
                c = [_hip.maxpool3s2(conv)]
                for i in range(4):
                    c.append(net.stage(i, c[-1]))
                r = {'prepare': timed(lambda: net.prepare(img)),
                     'stem_conv': timed(lambda: _hip.stem_conv7(x4, net.stem_w, net.stem_b)),
                     'max_pool': timed(lambda: _hip.maxpool3s2(conv))}
                for i in range(4):
                    r['stage%d' % (i + 1)] = timed(lambda i=i: net.stage(i, c[i]))
                r['fpn'] = timed(lambda: net.fpn(c[1:]))
                r['whole'] = timed(lambda: net.maps(img))
            r['whole_per_frame'] = round(r['whole'] / args.frames, 3)
            r['tmac_per_s'] = round(res['gmac_per_frame']['total'] * args.frames / r['whole'], 1)
            res[math + '_ms'] = r
    finally:
        cfg.config['convmath'] = old
    print(json.dumps(res))


if __name__ == '__main__':
    main()
