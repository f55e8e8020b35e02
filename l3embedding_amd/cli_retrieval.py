"""Cross-modal retrieval metrics of a trained AVC model over decoded clips.

    python -m l3embedding_amd.cli_retrieval WEIGHTS MODEL_TYPE CLIP.npz [CLIP.npz ...] [--output-path metrics.json]
                                            [--top-k K [--lists-path lists.npz]] [--maps-path maps.npz [--maps-top K]]

Each clip is an .npz holding `frames` (T, H, W, 3) uint8, `audio` (n,) or (n, C) int16 at 48 kHz and `rate` (avsample.load_clips).
Every whole second of every clip becomes one (frame, second) item; the metrics are recall@k, median rank and mean reciprocal
rank of the true partner among the items of the other clips, in both directions, and the AVC accuracy on the true pairs against as
many cross-clip pairs (crossmodal.evaluate_bank).  --top-k K adds what was retrieved: 'lists' in the JSON, per item and direction
the K best-scoring items of the other clips and the item's own partner, best first, as item indices (-1: none), clip ids and margins
(-inf is written as null); --lists-path also writes them as arrays, `frame_to_audio_index` ... `audio_to_frame_margin`, `item_clip`.
--maps-path FILE.npz adds 'peak' to the JSON -- the same metrics when a pair is scored by the best of the frame's 28 x 28 image
locations -- and writes `truth_map` (n, H, W), `truth_peak`, `truth_arg` (the location y W + x) of every true pair,
`peak_rank_v2a`, `peak_rank_a2v` and `item_clip`; with --maps-top K (<= --top-k) also `top_map` (n, K, H, W), `top_peak`, `top_arg`
of each frame's K retrieved seconds.
"""
import argparse
import json

import numpy as np

from . import avsample, crossmodal
from .model import load_model


def main(argv=None):
    p = argparse.ArgumentParser(prog='python -m l3embedding_amd.cli_retrieval', description=__doc__.split('\n')[0])
    p.add_argument('weights_path')
    p.add_argument('model_type')
    p.add_argument('clips', nargs='+')
    p.add_argument('--fps', type=int, default=30)
    p.add_argument('--recall-at', type=int, nargs='+', default=[1, 5, 10])
    p.add_argument('--batch-size', type=int, default=32)
    p.add_argument('--resize', type=int, default=256, help='0: the frames are already resized')
    p.add_argument('--seed', type=int, default=0, help='of the cross-clip pairs of the AVC accuracy')
    p.add_argument('--device', type=int, default=0)
    p.add_argument('--output-path', default=None, help='also write the metrics there as JSON')
    p.add_argument('--top-k', type=int, default=0, help='also list the K best-scoring items of every item, in both directions')
    p.add_argument('--lists-path', default=None, help='with --top-k: also write the lists there as .npz arrays')
    p.add_argument('--maps-path', default=None, help='also score every pair by its best image location and write the localisation '
                                                      'maps, peaks and peak locations of every true pair there as .npz arrays')
    p.add_argument('--maps-top', type=int, default=0, help='with --maps-path and --top-k: also those of each frame\'s K retrieved seconds')
    args = p.parse_args(argv)
    if args.lists_path and not args.top_k:
        p.error('--lists-path needs --top-k')
    if args.maps_top and not args.maps_path:
        p.error('--maps-top needs --maps-path')
    if not 0 <= args.maps_top <= args.top_k:
        p.error('--maps-top must be in [0, --top-k]')
    if not 0 <= args.top_k <= 64:
        p.error('--top-k must be in [1, 64]')
    pixels = samples = 0
    for path in args.clips:
        with np.load(path) as z:
            pixels += z['frames'].size
            samples += len(z['audio']) + 8
    model = load_model(args.weights_path, args.model_type)
    model.device = args.device
    bank = avsample.load_clips(avsample.ClipBank(args.device, pixels, samples, args.resize or None), args.clips)
    try:
        extra = {'peak': True, 'maps_top': args.maps_top} if args.maps_path else {}
        metrics = crossmodal.evaluate_bank(model, bank, fps=args.fps, ks=tuple(args.recall_at), batch_size=args.batch_size,
                                           seed=args.seed, topk=args.top_k, **extra)
        item_clip = crossmodal.retrieval_records(bank.clips, fps=args.fps)[1]
    finally:
        bank.close()
    if args.maps_path:
        maps = metrics.pop('maps')
        arrays = {'%s_%s' % (w, f): maps[w][f] for w in maps for f in maps[w]}
        for name in ('rank_v2a', 'rank_a2v'):
            arrays['peak_' + name] = metrics['peak'].pop(name)
        with open(args.maps_path, 'wb') as fh:
            np.savez(fh, item_clip=item_clip, **arrays)
    if args.top_k:
        lists = metrics['lists']
        if args.lists_path:
            arrays = {'%s_%s' % (d, f): lists[d][f] for d in lists for f in lists[d]}
            with open(args.lists_path, 'wb') as fh:
                np.savez(fh, item_clip=item_clip, **arrays)
        metrics['lists'] = {d: {'index': lists[d]['index'].tolist(), 'clip': lists[d]['clip'].tolist(),
                                'margin': [[float(m) if np.isfinite(m) else None for m in row] for row in lists[d]['margin']]}
                            for d in lists}
    text = json.dumps(metrics, indent=2, sort_keys=True)
    print(text)
    if args.output_path:
        with open(args.output_path, 'w') as fh:
            fh.write(text + '\n')
    return metrics


if __name__ == '__main__':
    main()
