"""Resident spectrograms (``tr_ds_to_memory: True``; reference NISQA_lib.py:2105-2127, served at :2165): the dB spectrogram of every
item of a SpeechQualityDataset, computed ONCE by the HIP front end and kept in HBM, so that an epoch reads no file -- DESIGN.md 6.4.

  arena      float32 [total_frames][48] on the device: the spectrograms as ``eng.mel(..., clamp=False)`` returns them, clip after clip
             in item order (a row is 192 B; a ten-second clip is 192 KB);
  floor      float32 [N] on the device: the clips' top_db floors;
  clip_row   int64 [N + 1], host and device: first arena row of every clip (exclusive prefix sum of ``frames``);
  frames, n_wins, sr, kind_i16   per clip on the host: spectrogram frames, segments, the file's sample rate and whether the host
             readers hand the file out as int16 (mono PCM16 / mono 16-bit FLAC) or as float32 -- what trainloop.stage_pairs orders by.

``fill()`` walks the dataset once through ingest.Ingest with the LengthAware policy and the device decoders, exactly as the predict
loop stages files (every WAV encoding, FLAC, ms_sr resampling).  The arena size comes from the header probe before anything is
allocated: one allocation, no growth, nothing spills to host memory.  ``NISQA_DS_MEMORY_BYTES`` caps the arena; unset, the cap is
half of the device memory free at that moment.  Under torchrun every rank fills its own complete store (batches are drawn from one
permutation over the whole set and every rank takes its share of each batch); nothing is exchanged between ranks.

``batch(ids)`` returns what train._FlatTrainer._mel_groups returns for the same clips -- (mel [frames][48], frame offsets on the
device, n_wins, clip floors) -- with ONE nisqa_mel_gather launch (csrc/melstore.hip) and one page-locked non-blocking upload of the
ids and the output offsets.
"""
import ctypes
import os
import time

import numpy as np
import torch

from . import ingest as _ingest
from . import lib as _lib
from .engine import BatchPlan
from .melbank import resampled_lengths

ROW_BYTES = 192                                     # 48 float32 mel bands


def host_kind_i16(info):
    """Which files of a header array the host readers (wavio.read_wav) return as int16: mono PCM in a 16-bit container and mono
    16-bit FLAC streams; everything else comes back as float32."""
    wav = (info['tag'] == _lib.WAV_TAG_PCM) & (info['channels'] == 1) & (info['block_align'] == 2)
    flac = (info['tag'] == _lib.WAV_TAG_FLAC) & (info['channels'] == 1) & (info['bits'] == 16)
    return wav | flac


def plans_from_headers(ds, info, names=None):
    """Header records of the items of ``ds`` (ingest.probe_headers) -> [(positions, BatchPlan)] per sample rate, by host arithmetic
    alone: the plan engine.HipNisqa.audio_plan gives the same files (at ms_sr when the dataset sets it, with the reference's
    'Sample too short' / 'n_wins > max_length' errors)."""
    srs, frames = info['sample_rate'].astype(np.int64), info['n_frames'].astype(np.int64)
    ms_sr = int(ds.ms_sr) if getattr(ds, 'ms_sr', None) is not None else None
    out = []
    for sr, pos in _ingest.rate_groups(srs):
        lengths, rate = frames[pos], sr
        if ms_sr is not None and sr != ms_sr:
            lengths, rate = resampled_lengths(lengths, sr, ms_sr)[0], ms_sr
        hop = int(rate * ds.ms_hop_length)                            # melbank.MelTables.hop
        out.append((pos, BatchPlan(lengths, hop, int(ds.seg_hop_length), ds.max_length,
                                   None if names is None else [names[k] for k in pos.tolist()])))
    return out


def memory_budget(device):
    """Bytes an arena may take: NISQA_DS_MEMORY_BYTES, else half of what torch.cuda.mem_get_info reports free right now."""
    env = os.environ.get('NISQA_DS_MEMORY_BYTES')
    if env is not None and env != '':
        return int(env)
    return int(torch.cuda.mem_get_info(device)[0]) // 2


def _alloc(rows, device):
    """THE allocation of a store: its arena [rows][48] float32."""
    return torch.empty((int(rows), 48), dtype=torch.float32, device=device)


class MelStore(object):
    def __init__(self, eng, ds):
        """eng: the HipNisqa whose mel front end computes the spectrograms (a HipNisqaDE's ``base``); ds: a SpeechQualityDataset or
        its ref_view().  Nothing is read or allocated before fill()."""
        self.eng, self.ds = eng, ds
        self.device = eng.device if eng is not None else None
        self.filled = False
        self.arena = self.floor = self.clip_row_dev = None
        self.clip_row = self.frames = self.n_wins = self.sr = self.kind_i16 = None

    def __len__(self):
        return len(self.ds)

    @property
    def nbytes(self):
        return int(self.clip_row[-1]) * ROW_BYTES

    # ---- layout from the headers ---------------------------------------------------------------------------------------
    def plan(self, num_workers=0):
        """Probe every header and lay the arena out (host only, nothing allocated) -> arena bytes.  A file whose header cannot be
        read raises the reference's ValueError('Could not load file ...')."""
        ds, n = self.ds, len(self.ds)
        names = ds.file_paths(range(n))
        info = _ingest.probe_headers(ds, range(n), num_workers)
        bad = np.flatnonzero(info['status'] != _lib.WAV_OK)
        if len(bad):
            raise ValueError('Could not load file {}'.format(names[int(bad[0])]))      # NISQA_lib.py:2305-2306
        self.frames, self.n_wins = np.zeros(n, np.int64), np.zeros(n, np.int32)
        for pos, p in plans_from_headers(ds, info, names):
            self.frames[pos], self.n_wins[pos] = p.T, p.n_wins
        self.sr = info['sample_rate'].astype(np.int64)
        self.kind_i16 = host_kind_i16(info)
        self.clip_row = np.concatenate(([0], np.cumsum(self.frames))).astype(np.int64)
        return self.nbytes

    # ---- the one pass over the files -----------------------------------------------------------------------------------
    def fill(self, num_workers=0):
        from . import NISQA_lib as NL
        t0 = time.perf_counter()
        need = self.plan(num_workers)
        allowed = memory_budget(self.device)
        if need > allowed:
            raise RuntimeError('tr_ds_to_memory: the spectrograms of {} clips need {} bytes of device memory, {} are allowed '
                               '(NISQA_DS_MEMORY_BYTES, or half of the free device memory); set tr_ds_to_memory: False to train '
                               'from the files'.format(len(self), need, allowed))
        eng, ds, n = self.eng, self.ds, len(self)
        self.arena = _alloc(self.clip_row[-1], self.device)
        self.floor = torch.empty(n, dtype=torch.float32, device=self.device)
        self.clip_row_dev = torch.from_numpy(self.clip_row).to(self.device)
        policy = _ingest.LengthAware(range(n), 1, lambda f, r: NL.tokens_of(ds, f, r), min_tokens=NL.MIN_TOKENS_SA,
                                     byte_cap=int(os.environ.get('NISQA_BATCH_BYTES', NL.BATCH_BYTE_CAP)))
        ing = _ingest.Ingest(ds, policy, pin=True, num_workers=num_workers, device=self.device,
                             device_decode=_ingest.device_decode_default(), device_flac=_ingest.device_flac_default())
        seen = np.zeros(n, dtype=bool)
        try:
            for staged in ing:
                raw = ing.ring.buf[staged.slot]
                ev = None
                try:
                    pcms = [_ingest.group_pcm(raw, g, eng, getattr(ds, 'ms_channel', None)) for g in staged.groups]
                    ev = torch.cuda.Event()
                    ev.record()                                       # behind the last group's copy
                finally:
                    ing.ring.release_after(staged.slot, ev)
                for g, pcm in zip(staged.groups, pcms):
                    plan = eng.audio_plan(g.lengths, g.sr, names=g.names)
                    pcm = eng.resample(pcm, g.lengths, g.sr)         # a no-op unless ms_sr is set and differs from the files' rate
                    mel, floor = eng.mel(pcm, plan, eng.rate(g.sr), clamp=False)
                    ids = np.asarray(g.ids, dtype=np.int64)
                    if (plan.T != self.frames[ids]).any() or seen[ids].any():
                        k = int(np.flatnonzero((plan.T != self.frames[ids]) | seen[ids])[0])
                        raise RuntimeError('tr_ds_to_memory: {} changed while the store was filled'.format(g.names[k]))
                    seen[ids] = True
                    for k, i in enumerate(ids.tolist()):              # device-to-device, into the clip's rows
                        self.arena[self.clip_row[i]:self.clip_row[i + 1]].copy_(mel[plan.frame_off[k]:plan.frame_off[k + 1]])
                    self.floor.index_copy_(0, torch.from_numpy(ids).to(self.device), floor)
            if not seen.all():
                raise RuntimeError('tr_ds_to_memory: {} of {} clips were not staged'.format(int((~seen).sum()), n))
            torch.cuda.synchronize(self.device)
        finally:
            ing.close(keep_ring=False)                               # ring, readers: nothing of the file feed stays behind
        self.filled = True
        self.eng = None                                              # the front end is not needed again (its model may be rebuilt)
        self.lib = _lib.load()
        print('tr_ds_to_memory: {} clips, {} frames, {} bytes on {}, {:.2f} s'.format(n, int(self.clip_row[-1]), self.nbytes,
                                                                                     self.device, time.perf_counter() - t0))
        return self

    # ---- batches ---------------------------------------------------------------------------------------------------------
    def kinds(self, ids):
        """[(sample rate, numpy dtype string of the host readers' samples)] of the items ``ids``: trainloop.pair_order's keys."""
        return [(int(self.sr[i]), '<i2' if self.kind_i16[i] else '<f4') for i in ids]

    def check_table(self, ids, out_frame_off):
        """The host half of nisqa_mel_gather's contract: every id in range, every output span the stored length."""
        ids, off = np.asarray(ids).reshape(-1), np.asarray(out_frame_off).reshape(-1)
        if len(ids) == 0 or len(off) != len(ids) + 1:
            raise ValueError('a batch needs at least one id and one more output offset than ids')
        for c, i in enumerate(ids.tolist()):
            if not 0 <= i < len(self):
                raise ValueError('entry {}: id {} is outside the store of {} clips'.format(c, i, len(self)))
            if int(off[c + 1]) - int(off[c]) != int(self.frames[i]):
                raise ValueError('entry {}: output span {} is not the {} stored frames of clip {}'.format(
                    c, int(off[c + 1]) - int(off[c]), int(self.frames[i]), i))
        if int(off[0]) != 0 or int(off[-1]) >= 2 ** 31:
            raise ValueError('output offsets must start at 0 and stay below 2^31 frames, got {} .. {}'.format(int(off[0]), int(off[-1])))

    def gather(self, ids, out_frame_off, out_mel=None, out_floor=None):
        """One nisqa_mel_gather launch on the current stream -> (out_mel [frames][48], device frame offsets int32 [n + 1],
        out_floor [n]); out_mel / out_floor: device buffers to write (default: new ones)."""
        self.check_table(ids, out_frame_off)
        n, total = len(ids), int(out_frame_off[-1])
        host = torch.empty(2 * n + 1, dtype=torch.int32, pin_memory=True)     # page-locked + non-blocking, like engine.resample's tables
        hv = host.numpy()
        hv[:n], hv[n:] = ids, out_frame_off
        dev = host.to(self.device, non_blocking=True)
        if out_mel is None:
            out_mel = torch.empty((total, 48), dtype=torch.float32, device=self.device)
        if out_floor is None:
            out_floor = torch.empty(n, dtype=torch.float32, device=self.device)
        assert out_mel.is_contiguous() and out_mel.numel() == total * 48 and out_floor.is_contiguous() and out_floor.numel() == n
        st = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(self.lib.nisqa_mel_gather(self.arena.data_ptr(), int(self.clip_row[-1]), self.clip_row_dev.data_ptr(),
                                             self.floor.data_ptr(), len(self), dev.data_ptr(), dev.data_ptr() + 4 * n, n, total,
                                             out_mel.data_ptr(), out_floor.data_ptr(), st), 'nisqa_mel_gather')
        return out_mel, dev[n:], out_floor

    def offsets(self, ids):
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        if len(ids) and ((ids < 0) | (ids >= len(self))).any():
            c = int(np.flatnonzero((ids < 0) | (ids >= len(self)))[0])
            raise ValueError('entry {}: id {} is outside the store of {} clips'.format(c, int(ids[c]), len(self)))
        return ids, np.concatenate(([0], np.cumsum(self.frames[ids]))).astype(np.int64)

    def batch(self, ids):
        """ids already in step order -> (mel [frames][48], frame offsets on the device, n_wins, clip floors): the four things
        train._FlatTrainer._mel_groups returns for these clips."""
        ids, off = self.offsets(ids)
        mel, off_dev, floor = self.gather(ids, off)
        return mel, off_dev, self.n_wins[ids].astype(np.int32), floor

    def item(self, index):
        """(dB spectrogram [T][48] with the top_db floor applied, n_wins) of one clip, on the host: what the reference serves from
        memory at NISQA_lib.py:2165."""
        a, b = int(self.clip_row[index]), int(self.clip_row[index + 1])
        spec = np.maximum(self.arena[a:b].cpu().numpy(), self.floor[index:index + 1].cpu().numpy()[0])
        return spec, int(self.n_wins[index])


def batch_plan(n_wins, frames):
    """The BatchPlan of clips whose spectrograms lie back to back (frames[b] rows each): what the engine's stage API (cnn / cnn_std,
    td_pool / lstm, forward_features) needs next to (mel, floor)."""
    plan = BatchPlan.from_n_wins(n_wins)
    plan.T = np.asarray(frames, dtype=np.int64)
    plan.frame_off = np.concatenate(([0], np.cumsum(plan.T))).astype(np.int32)
    plan.total_frames = int(plan.frame_off[-1])
    return plan


def work_batches(tokens, bs, min_tokens, min_clips=1):
    """Batches of a resident dataset cut by work, as ingest.LengthAware cuts file batches: the items sorted by length, a batch
    closed once it holds at least ``bs`` clips, ``min_clips`` clips and ``min_tokens`` segments (rows do not depend on the batch
    composition) -> lists of positions."""
    tokens = np.asarray(tokens, dtype=np.int64)
    order = np.lexsort((np.arange(len(tokens)), tokens))
    need = max(1, int(bs), int(min_clips))
    out, cur, ct = [], [], 0
    for k in order.tolist():
        cur.append(k)
        ct += int(tokens[k])
        if len(cur) >= need and ct >= min_tokens:
            out.append(cur)
            cur, ct = [], 0
    if cur:
        out.append(cur)
    return out
