"""The BRIR files of one measurement from its compact PCM words (the job runners' output="pcm").

The reference ends by writing files: `_stage_write_brirs` (core/pipeline.py:865-876) writes hrir.wav in
HEXADECAGONAL_TRACK_ORDER and hesuvi.wav in HESUVI_TRACK_ORDER, and `_stage_truehd_layouts` (:878-906) the TrueHD layouts,
all through HRIR.write_wav: PCM words of the responses in the file's track order, silent tracks for absent channels.  The
device quantises the slice's rows once (imp_slice_pack_pcm: the rule HRIR.write_wav's files are written with), in slice
column order; a file is then one scatter of those columns into its track order.
"""
import os

import numpy as np

from .audio_io import pcm_quantise, write_wav, write_wav_frames
from .constants import (HESUVI_TRACK_ORDER, HEXADECAGONAL_TRACK_ORDER, TRUEHD_11CH_ORDER, TRUEHD_13CH_ORDER,
                        track_name)

# (name, channel order, minimum channel count) of core/pipeline.py:885-888: 7.0.4 and 7.0.6
TRUEHD_LAYOUTS = (("11ch", TRUEHD_11CH_ORDER, 8), ("13ch", TRUEHD_13CH_ORDER, 10))


def check_bit_depth(bit_depth):
    if isinstance(bit_depth, (bool, np.bool_)) or bit_depth not in (16, 24, 32):
        raise ValueError(f"bit_depth must be 16, 24 or 32, got {bit_depth!r}")
    return int(bit_depth)


class BrirFrames:
    """One measurement's responses as PCM words: frames int32 [n, R], column c = track `tracks[c]` (slice row order:
    speaker q, side s at 2 q + s), each word clip(lrint(x * 2^31), -2^31, 2^31 - 1) >> (32 - bit_depth).  `frames` may be a
    view of a page-locked block of a runner's pool: the block goes back to the pool when the last view is dropped."""

    def __init__(self, fs, bit_depth, tracks, frames):
        self.fs = int(fs)
        self.bit_depth = check_bit_depth(bit_depth)
        self.tracks = list(tracks)
        self.frames = frames
        if frames.ndim != 2 or frames.shape[1] != len(self.tracks) or frames.dtype != np.int32:
            raise ValueError(f"frames must be int32 [n, {len(self.tracks)}], got {frames.dtype} {frames.shape}")
        self.speakers = list(dict.fromkeys(t.rsplit("-", 1)[0] for t in self.tracks))

    @classmethod
    def from_hrir(cls, hrir, tasks, bit_depth):
        """the words of an HRIR's responses (tasks: [(speaker, side)] in column order), quantised by the host codec"""
        rows = np.stack([np.asarray(hrir.irs[sp][sd].data, dtype=np.float64) for sp, sd in tasks], axis=1)
        words = pcm_quantise(rows, check_bit_depth(bit_depth)).astype(np.int32)
        return cls(hrir.fs, bit_depth, [track_name(sp, sd) for sp, sd in tasks], words)

    def __len__(self):
        return self.frames.shape[0]

    def _columns(self, track_order):
        col = {t: c for c, t in enumerate(self.tracks)}
        pairs = [(k, col[t]) for k, t in enumerate(track_order) if t in col]
        return [k for k, _ in pairs], [c for _, c in pairs]

    def data_chunk(self, track_order=None):
        """the WAV data chunk's words [n, len(track_order)]: the columns in the file's track order, zeros for absent tracks"""
        order = HEXADECAGONAL_TRACK_ORDER if track_order is None else track_order
        dst, src = self._columns(order)
        out = np.zeros((len(self), len(order)), dtype=np.int32)
        out[:, dst] = self.frames[:, src]
        return out

    def write_wav(self, file_path, track_order=None):
        """the file HRIR.write_wav(file_path, track_order, bit_depth) writes for the same responses, byte for byte"""
        order = HEXADECAGONAL_TRACK_ORDER if track_order is None else track_order
        if len(self) <= len(order):
            # the reference's rule for data with fewer frames than tracks (core/audio_io.py:82-97 transposes it): the host
            # codec on the exact float values of the words
            rows = np.zeros((len(order), len(self)))
            dst, src = self._columns(order)
            rows[dst] = self.frames[:, src].T.astype(np.float64) * 2.0 ** (32 - self.bit_depth - 31)
            write_wav(file_path, self.fs, rows, bit_depth=self.bit_depth)
            return
        write_wav_frames(file_path, self.fs, self.data_chunk(order), self.bit_depth)

    def write_brirs(self, dir_path, truehd=False):
        """hrir.wav and hesuvi.wav in dir_path (core/pipeline.py:865-876); truehd: also truehd_{11ch|13ch}_{k}ch.wav for the
        layouts with enough channels present (:878-906; a layout with too few is skipped).  Returns the paths written."""
        paths = [os.path.join(dir_path, "hrir.wav"), os.path.join(dir_path, "hesuvi.wav")]
        self.write_wav(paths[0])
        self.write_wav(paths[1], track_order=HESUVI_TRACK_ORDER)
        if truehd:
            for name, layout_order, min_channels in TRUEHD_LAYOUTS:
                available = [ch for ch in layout_order if ch in self.speakers]
                if len(available) < min_channels:
                    continue
                paths.append(os.path.join(dir_path, f"truehd_{name}_{len(available)}ch.wav"))
                self.write_wav(paths[-1], track_order=[track_name(ch, sd) for ch in available for sd in ("left", "right")])
        return paths
