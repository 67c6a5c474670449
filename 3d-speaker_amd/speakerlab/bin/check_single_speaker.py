"""Single-speaker check — drop-in for ``speakerlab/bin/check_single_speaker.py``.

Same arguments and output layout as the reference: ``--wav`` (a wav, or a text file with one path
per line) or ``--src_dir`` with ``--pattern``; per file VAD, one embedding per speech segment, the
cosine of every segment pair, and ``is_single_speaker = min >= threshold``.  Directory mode writes
``<base>.single_spk.json`` per file into ``--out_dir``; list mode writes one object (or a list) to
``--out`` or stdout.

The reference reads its segments from a VAD interface its own tree no longer has; here a file's
segments are the refined VAD intervals of the diarization front end
(``Diarization3Dspeaker.last_vad_time``, ``no_chunk_after_vad``), each circle-padded to the file's
longest one as the reference does.

MI355X execution: ``--files_per_batch K`` files go through the front end, their segments are
embedded in shared batches (``do_emb_extraction_pooled``), the embeddings stay on the device, one
``spk_pair_cosine_stats`` call gives every file's pair cosines, minimum and mean, and one copy
brings them back.
"""
import argparse
import json
import os
import sys

_PKG = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

from speakerlab.utils import single_speaker  # noqa: E402


def build_parser():
    parser = argparse.ArgumentParser(
        description='Check if utterances are single-speaker via VAD + embeddings; supports batch mode.')
    group = parser.add_mutually_exclusive_group(required=True)
    group.add_argument('--wav', help='Path to a WAV file or a text file (one path per line)')
    group.add_argument('--src_dir', help='Directory to scan for wavs (use with --pattern)')
    parser.add_argument('--pattern', default='*speech_estimate.wav', help='Filename pattern when using --src_dir')
    parser.add_argument('--threshold', type=float, default=0.8,
                        help='Cosine similarity threshold for single-speaker decision')
    parser.add_argument('--out', default=None, help='JSON output path for single-file/list mode')
    parser.add_argument('--out_dir', default=None,
                        help='Output directory for batch mode; per-file JSONs will be written here')
    parser.add_argument('--files_per_batch', default=16, type=int, metavar='K',
                        help='MI355X build: files whose segments are embedded in shared batches and scored by '
                             'one pair-statistics call; 1: every file on its own')
    parser.add_argument('--batch_size', default=64, type=int, help='Segments per embedding batch')
    parser.add_argument('--gpu_vad', action='store_true',
                        help='MI355X build: VAD frame energies on the GPU (HIP kernels), the signal uploaded once')
    parser.add_argument('--gpu_resample', action='store_true',
                        help='MI355X build: resample non-16 kHz input on the GPU')
    parser.add_argument('--vad', choices=['auto', 'ten_vad', 'energy'], default='auto',
                        help='MI355X build: VAD engine (TenVad when importable, else the energy stand-in)')
    parser.add_argument('--synthetic_weights', action='store_true',
                        help='MI355X build: deterministic random weights instead of a checkpoint (no network)')
    parser.add_argument('--model_cache_dir', default='pretrained', type=str,
                        help='MI355X build: directory holding iic/speech_eres2netv2_sv_zh-cn_16k-common/<ckpt>')
    parser.add_argument('--no_pairs', action='store_true',
                        help='MI355X build: leave pairwise_similarities out of the results; the pair cosines are '
                             'then never written to memory')
    return parser


def input_paths(args):
    """(paths, directory mode) of the parsed arguments, as the reference resolves them."""
    if args.src_dir:
        from glob import glob
        src_dir = os.path.abspath(args.src_dir)
        paths = sorted(glob(os.path.join(src_dir, args.pattern)))
        if not paths:
            raise SystemExit(f'No files matched pattern `{args.pattern}` under {src_dir}')
        return paths, True
    if args.wav.endswith('.wav'):
        return [args.wav], False
    with open(args.wav, 'r') as f:
        return [line.strip() for line in f if line.strip()], False


def output_dir(args):
    """Directory mode's output folder: ``--out_dir``, else ``single_spk_check`` under the source."""
    return args.out_dir or os.path.join(os.path.abspath(args.src_dir), 'single_spk_check')


def output_file(out_dir, wav_path):
    """Directory mode's per-file name: ``<base>.single_spk.json``."""
    return os.path.join(out_dir, os.path.splitext(os.path.basename(wav_path))[0] + '.single_spk.json')


class SingleSpeakerChecker:
    """VAD -> one embedding per speech segment -> pair cosines, minimum and mean on the device.

    ``check(wav)`` returns the reference's result dict for one file, ``check_many(wavs)`` the list
    of them for a group of files handled together; ``check_many(ws) == [check(w) for w in ws]``."""

    def __init__(self, device=None, threshold=0.8, batch_size=64, gpu_vad=False, gpu_resample=False, vad='auto',
                 synthetic_weights=False, model_cache_dir=None, want_pairs=True):
        from speakerlab.bin.infer_diarization import Diarization3Dspeaker
        self.front = Diarization3Dspeaker(device, model_cache_dir=model_cache_dir, no_chunk_after_vad=True,
                                          batch_size=batch_size, synthetic_weights=synthetic_weights, vad=vad,
                                          gpu_resample=gpu_resample, gpu_vad=gpu_vad)
        self.device = self.front.device
        self.threshold = float(threshold)
        self.want_pairs = bool(want_pairs)

    def check(self, wav):
        return self.check_many([wav])[0]

    def check_many(self, wavs):
        wavs = list(wavs)
        segments, signals = [], []
        for wav in wavs:
            chunks, wav_data = self.front.do_front(wav)
            segments.append([[float(st), float(ed)] for st, ed in chunks])
            signals.append(wav_data)
        embeddings = self.front.do_emb_extraction_pooled(segments, signals, keep_on_device=True)
        stats = single_speaker.pair_stats(embeddings, self.threshold, want_cos=self.want_pairs)
        return [single_speaker.make_result(w if isinstance(w, str) else None, seg, self.threshold, st,
                                           self.want_pairs)
                for w, seg, st in zip(wavs, segments, stats)]


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.files_per_batch < 1:
        raise SystemExit('--files_per_batch must be at least 1')
    paths, directory_mode = input_paths(args)
    if not paths:
        raise SystemExit(f'{args.wav} lists no files')
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError('the MI355X build runs the single-speaker check on a ROCm device only')
    checker = SingleSpeakerChecker(torch.device('cuda'), threshold=args.threshold, batch_size=args.batch_size,
                                   gpu_vad=args.gpu_vad, gpu_resample=args.gpu_resample, vad=args.vad,
                                   synthetic_weights=args.synthetic_weights, model_cache_dir=args.model_cache_dir,
                                   want_pairs=not args.no_pairs)
    groups = [paths[lo:lo + args.files_per_batch] for lo in range(0, len(paths), args.files_per_batch)]
    if directory_mode:
        # every group's files are written when the group is done; nothing is kept
        out_dir = output_dir(args)
        os.makedirs(out_dir, exist_ok=True)
        for group in groups:
            for p, res in zip(group, checker.check_many(group)):
                with open(output_file(out_dir, p), 'w') as f:
                    json.dump(res, f, indent=2, ensure_ascii=False)
        print(f'[INFO] Wrote {len(paths)} results to {out_dir}')
        return None
    # list mode writes one JSON value, so it holds the list's results (--no_pairs keeps them small)
    results = [res for group in groups for res in checker.check_many(group)]
    one = results if len(results) > 1 else results[0]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(one, f, indent=2, ensure_ascii=False)
    else:
        print(json.dumps(one, indent=2, ensure_ascii=False))
    return results


if __name__ == '__main__':
    main()
