"""Diagnostic: per-phase cycle counts of the lean 52 -> 52 fp16x3 halo conv (conv3x3_halo.hip built
with -DSPK_HALO_PROF=1 into a separate library: tools/variant_lib.sh haloprof
3d-speaker_amd/csrc/conv3x3_halo.hip -DSPK_HALO_PROF=1, then SPK_HIP_LIB=ablibs/libspk_haloprof.so).
One launch per arm at the ERes2NetV2 layer-2 shape (256 x 40 x 99, tile width 16), without and
with the Res2Net addend, on the sliced form (SPK_HALO_WHOLE_N=0) and the whole-N form (=1); prints
mean cycles per tile per phase over waves."""
import ctypes
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, '3d-speaker_amd'), os.path.join(REPO, 'tests')]
import numpy as np  # noqa: E402
import torch  # noqa: E402

PH = ['issue+taps', 'bar-taps', 'partials->LDS', 'bar-partials', 'epilogue', 'bar-epi/stores', 'staging', 'bar-stage']


def main():
    import conv_cases
    from speakerlab import _hip
    dev = torch.device('cuda', 0)
    be = conv_cases.Backend(_hip.lib(), dev, emu=False)
    prof = ctypes.CDLL(_hip.LIB_PATH).spk_exp_halo_prof
    nimg, H, W = 256, 40, 99
    tiles = nimg * ((H + 7) // 8) * ((W + 15) // 16)
    for whole in (0, 1):
        os.environ['SPK_HALO_WHOLE_N'] = str(whole)
        for add in (0, 1):
            c = conv_cases.case(f'prof_{whole}_{add}', 'halo_x3', '', nimg=nimg, H=H, W=W, cin=52, N=52, k=(3, 3), add=add)
            g, t = conv_cases.build(c)
            keep = []
            d, out, _, _ = conv_cases.descriptor(c, g, t, be, keep)
            for _ in range(3):
                rc, kernel, err = conv_cases.conv_diag.launch(be.handle, d)
                assert rc == 0, err
                torch.cuda.synchronize()
            n = 512 * 8 * 8
            buf = (ctypes.c_longlong * n)()
            assert prof(buf, n) == 0
            a = np.frombuffer(buf, dtype=np.int64).reshape(512, 8, 8)
            blocks = min(tiles, torch.cuda.get_device_properties(dev).multi_processor_count)   # both forms' grid
            used = a[:blocks].astype(np.float64)
            # cycles per output tile, waves averaged (the sliced form: both slices of the tile)
            per_tile = used.sum(axis=0).mean(axis=0) / tiles
            tot = per_tile.sum()
            print(f'{kernel}  ({tiles} tiles, {blocks} blocks)')
            for i, p in enumerate(PH):
                print(f'  {p:16s} {per_tile[i]:9.0f} cycles/tile {100 * per_tile[i] / tot:5.1f}%')
            print(f'  total {tot:.0f} cycles per tile; longest wave {used.sum(axis=2).max():.0f} cycles')
            del keep, d, out


if __name__ == '__main__':
    main()
