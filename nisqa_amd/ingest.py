"""Host ingest of the predict loop: WAV files -> page-locked staging -> one H2D copy per batch.

The kernels take ~1 ms for a batch of 64 ten-second clips, i.e. 60 GB/s of PCM16; a loader that builds a Python
``bytes`` per file, slices it, concatenates the batch and pins the result (five copies per sample) feeds them at
1.7 k clips/s, and Python threads doing the reads themselves stop at ~8 k (interpreter lock).  Here a sample is
copied ONCE on the host and no Python runs per file: libnisqa_ingest.so (csrc/ingest.cpp, include/nisqa_ingest.h)
parses the RIFF headers of the whole batch on a native thread pool, the batch layout is fixed from the headers
alone, and the same pool then ``pread``-s every data chunk straight into its slice of a persistent page-locked
buffer (page cache -> pinned memory).  Three such buffers rotate: one being filled by the producer thread, one in flight over PCIe, one spare;
a slot is recycled only after the HIP event recorded behind its H2D copy has completed.

Files that are not mono PCM16 (stereo, 8/24/32-bit, float, G.711, RIFX) take one of two roads.  With ``device_decode`` (what the
predict and the training loop ask for) their data chunks are copied VERBATIM like the mono PCM16 ones, the rate group travels as raw
bytes with a table of ``nisqa_wav_clip`` records, and ``nisqa_wav_decode`` turns it into float32 mono samples on the GPU
(``group_pcm``): no Python runs per sample.  Without it (the default of ``Ingest``, and ``NISQA_HOST_DECODE=1`` in the loops) they
are decoded by ``wavio.read_wav`` with the reference's ``lb.load`` semantics and staged as float32 through the same buffers.  FLAC
files (lb.load reads them through the same soundfile call) are decoded by the native reader threads: mono 16-bit streams straight
into their int16 slot, others via ``wavio`` -- unless the loop also asks for ``device_flac``: then the threads only copy the frame region
of a fixed-block-size stream (first audio frame to end of file, about half the bytes of its PCM) and index its frames, the group
travels as a 'flac' group, and ``nisqa_flac_decode`` decodes it on the GPU, one lane per frame, every CRC and the MD5 checked there.
"""
import ctypes
import os
import queue
import threading
import time

import numpy as np
import torch

from . import lib as _lib
from . import wavio

_ALIGN = 64
_RAW_ALIGN = 16                                    # nisqa_wav_decode: every data chunk of a raw group starts on a 16-byte boundary
WAV_CLIP = np.dtype(_lib.WavClip)                  # one row of a raw group's table (nisqa_wav_clip)
FLAC_CLIP = np.dtype(_lib.FlacClip)                # one row of a flac group's device table (nisqa_flac_clip)
FLAC_PLAN = np.dtype(_lib.FlacPlan)                # nisqa_flac_plan
FLAC_FRAME = np.dtype(_lib.FlacFrame)              # nisqa_flac_frame
_noted = set()


def _note_once(msg):
    if msg not in _noted:
        _noted.add(msg)
        print(msg)


def cpu_budget():
    """CPUs this process may actually burn: the affinity mask, cut down to the cgroup's CPU quota (cpu.max of cgroup v2,
    cpu.cfs_quota_us of v1).  A container with 256 visible cores and a 16-CPU quota that starts 32 reader threads spends
    its quota in half of every 100 ms period and is then frozen for the other half -- consumer thread included."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1)
    try:
        with open('/sys/fs/cgroup/cpu.max') as f:
            quota, period = f.read().split()[:2]
        if quota != 'max':
            n = min(n, max(1, int(quota) // int(period)))
    except (OSError, ValueError):
        try:
            with open('/sys/fs/cgroup/cpu/cpu.cfs_quota_us') as f:
                quota = int(f.read())
            with open('/sys/fs/cgroup/cpu/cpu.cfs_period_us') as f:
                period = int(f.read())
            if quota > 0:
                n = min(n, max(1, quota // period))
        except (OSError, ValueError):
            pass
    return n


def gpu_local_cpus(device):
    """CPUs of the NUMA node the GPU hangs off (sysfs local_cpulist of its PCI function), cut to this process's affinity
    mask; empty set when unknown.  Reader threads that copy page-cache pages into the page-locked staging buffer run
    1.5x faster on the GPU's own node (2.2 against 3.4 ms per 245 MB batch), and with eight ranks on a two-socket host
    it keeps every rank's staging traffic off the inter-socket links."""
    try:
        p = torch.cuda.get_device_properties(device)
        path = '/sys/bus/pci/devices/%04x:%02x:%02x.0/local_cpulist' % (p.pci_domain_id, p.pci_bus_id, p.pci_device_id)
        with open(path) as f:
            txt = f.read().strip()
        cpus = set()
        for part in txt.split(','):
            if '-' in part:
                a, b = part.split('-')
                cpus.update(range(int(a), int(b) + 1))
            elif part:
                cpus.add(int(part))
        return cpus & set(os.sched_getaffinity(0))
    except Exception:
        return set()


def probe_headers(ds, indices, num_workers=0):
    """RIFF header records (numpy structured array of lib.WavInfo: status, n_frames, sample_rate, ...) of the items
    ``indices`` of a SpeechQualityDataset, native threads, headers only.  Nothing is raised for an unreadable file: its
    ``status`` says so (the work-balanced shards of the predict loop only need lengths; the reference's ValueError is
    raised where the reference raises it, when the file is loaded)."""
    idx = list(indices)
    n = len(idx)
    col, d = ds.df[ds.filename_column].tolist(), ds.data_dir
    enc = [os.fsencode(os.path.join(d, col[i])) for i in idx]
    paths = (ctypes.c_char_p * n)(*enc)
    infos = (_lib.WavInfo * n)()
    asked = int(num_workers or 0)
    try:
        local_world = max(1, int(os.environ.get('LOCAL_WORLD_SIZE', '1')))
    except ValueError:
        local_world = 1
    budget = max(1, cpu_budget() // local_world)
    workers = max(1, min(asked if asked > 0 else budget, budget))
    _lib.load_ingest().nisqa_ingest_probe(paths, n, infos, workers)
    return np.ctypeslib.as_array(infos).copy()


def _verbatim_i16(info):
    """Which files of a header array reach the staging buffer as int16: mono PCM16 data chunks (copied verbatim) and mono 16-bit
    FLAC streams (decoded into the slot by the reader threads, csrc/flac.hpp)."""
    return ((info['tag'] == _lib.WAV_TAG_PCM) | (info['tag'] == _lib.WAV_TAG_FLAC)) & (info['bits'] == 16) & (info['channels'] == 1)


class StagingRing(object):
    """``n_slots`` page-locked byte buffers, grown on demand.  A slot handed to the consumer comes back with
    ``release_after(slot, event)``; ``acquire`` blocks until then and until ``event`` (the HIP event recorded
    behind the slot's H2D copies) has completed."""

    def __init__(self, n_slots, pin):
        self.pin = pin
        self.buf = [None] * n_slots
        self.busy = [None] * n_slots
        self.back = [threading.Event() for _ in range(n_slots)]
        for e in self.back:
            e.set()
        self.k = 0

    def acquire(self, nbytes):
        k = self.k
        self.k = (k + 1) % len(self.buf)
        self.back[k].wait()
        if self.busy[k] is not None:
            self.busy[k].synchronize()
            self.busy[k] = None
        if self.buf[k] is None or self.buf[k].numel() < nbytes:
            self.buf[k] = None
            self.buf[k] = torch.empty(nbytes + nbytes // 4 + 4096, dtype=torch.uint8, pin_memory=self.pin)
        self.back[k].clear()
        return k

    def release_after(self, k, event):
        self.busy[k] = event
        self.back[k].set()

    def abandon(self):
        for e in self.back:
            e.set()

    def reset(self):
        """Ready for a new loop: every slot free (after the copies still reading from it), buffers kept."""
        for k in range(len(self.buf)):
            if self.busy[k] is not None:
                self.busy[k].synchronize()
                self.busy[k] = None
            self.back[k].set()
        self.k = 0
        return self


# Page-locking a few hundred MB costs tens of milliseconds per buffer: the rings of finished loops are kept for the next
# one (one predict() call per process is the common case, repeated calls and the train/validate alternation the other).
_spare_rings = {}
_spare_lock = threading.Lock()


def _take_ring(n_slots, pin):
    with _spare_lock:
        lst = _spare_rings.get((n_slots, pin))
        if lst:
            return lst.pop().reset()
    return StagingRing(n_slots, pin)


def _give_ring(ring):
    with _spare_lock:
        lst = _spare_rings.setdefault((len(ring.buf), ring.pin), [])
        if len(lst) < 2:
            lst.append(ring)


class Group(object):
    """Clips of one sample rate inside a staged batch.  ``kind``: 'i16' (mono PCM16 back to back), 'f32' (host-decoded float32 back to
    back) or 'raw' (data chunks as the files hold them, each on a 16-byte boundary, ``nbytes`` of them from ``offset`` on; ``clips``
    is then the nisqa_wav_clip table, a numpy structured array of dtype WAV_CLIP whose src_off counts from ``offset`` and whose dst_off
    is the clip's sample offset in the decoded group).  A 'flac' group is a raw group some of whose clips are FLAC frame regions for
    the device decoder: ``flac`` is then a dict -- 'clips' (the nisqa_flac_clip table of those clips, src_off from ``offset``),
    'pos' (their positions in the group), 'frames_off' / 'n_rows' (the nisqa_flac_frame rows behind the clips' bytes), 'as_i16' (every
    clip of the group is mono 16-bit: the group decodes to int16) -- and ``clips`` holds the rows of the other clips only; ``status``
    receives the device status words when the group is decoded.  ``lengths`` are frames in every kind."""
    __slots__ = ('ids', 'lengths', 'sr', 'offset', 'nbytes', 'is_i16', 'names', 'kind', 'clips', 'flac', 'status')

    def __init__(self, ids, lengths, sr, offset, nbytes, is_i16, names=None, kind=None, clips=None, flac=None):
        self.ids, self.lengths, self.sr, self.offset, self.nbytes, self.is_i16 = ids, lengths, sr, offset, nbytes, is_i16
        self.names = names
        self.kind = kind if kind is not None else ('i16' if is_i16 else 'f32')
        self.clips = clips
        self.flac, self.status = flac, None


class Staged(object):
    __slots__ = ('slot', 'groups')

    def __init__(self, slot, groups):
        self.slot, self.groups = slot, groups


def rate_groups(srs):
    """The groups one staged batch falls into: one per sample rate, in order of first appearance, batch order inside a group ->
    [(rate, positions)].  Ingest._stage_once lays a batch out by it and the resident training loop (melstore) draws its batches by
    it, so both enter the step in the same clip order."""
    srs = np.asarray(srs)
    return [(int(sr), np.flatnonzero(srs == sr)) for sr in dict.fromkeys(srs.tolist())]


def step_order(srs):
    """Positions of a batch's clips in the order the training step sees them: rate_groups, group after group."""
    return np.concatenate([pos for _, pos in rate_groups(srs)]) if len(srs) else np.zeros(0, dtype=np.int64)


class LengthAware(object):
    """Batching policy of the predict loop: the producer probes the RIFF headers of a
    window of items (headers only, native threads), sorts the window by (sample rate, length) and cuts batches by WORK,
    not by a clip count -- a batch is closed when it holds at least ``bs`` clips AND at least ``min_clips`` clips AND at
    least ``min_tokens`` segments, or when the next clip would push its staged bytes over ``byte_cap``.

    ``bs`` (the reference's --bs / tr_bs_val) is therefore a LOWER bound: the reference's default ``--bs 1`` coalesces
    into full launches (results do not depend on the batch composition: eval-mode BatchNorm, per-clip masks; tested), and
    clips of similar length share a batch, so a launch of the BiLSTM (as long as its longest clip) or of the attention
    kernels carries no short clips waiting for a long one.  The consumer scatters result rows back by item index, so the
    output order is the input order.

    tokens_of(n_frames[int64 array], sample_rate[int array]) -> segments per clip (host arithmetic on header fields)."""

    def __init__(self, indices, bs, tokens_of, min_tokens=0, min_clips=1, byte_cap=256 << 20, window=16384):
        self.indices = list(indices)
        self.bs, self.tokens_of = max(1, int(bs)), tokens_of
        self.min_tokens, self.min_clips = int(min_tokens), max(1, int(min_clips))
        self.byte_cap, self.window = int(byte_cap), max(1, int(window))

    def __len__(self):
        return len(self.indices)

    @staticmethod
    def staged_bytes(frames, srs, widths, pos):
        """Bytes Ingest._stage lays out for the clips ``pos`` when it decodes on the host: clips of one sample rate form a group, and a
        group is staged as int16 only if ALL its clips are mono PCM16 (width 2) -- one stereo / 24-bit / float / G.711 file widens
        its whole group to float32."""
        pos = np.asarray(pos, dtype=np.int64)
        total = 0
        for sr in np.unique(srs[pos]):
            sel = pos[srs[pos] == sr]
            total += int(frames[sel].sum()) * (2 if (widths[sel] == 2).all() else 4)
        return total

    @staticmethod
    def raw_bytes(frames, widths, pos):
        """Bytes Ingest._stage lays out for the clips ``pos`` with device decode: every clip at its own staged width (``widths``:
        block_align of a verbatim data chunk, 4 of a host-decoded entry), each on a 16-byte boundary.  (A group of mono PCM16 clips
        alone is packed without the pads: at most 15 bytes per clip less.)"""
        pos = np.asarray(pos, dtype=np.int64)
        return int(((frames[pos] * widths[pos] + _RAW_ALIGN - 1) // _RAW_ALIGN * _RAW_ALIGN).sum())

    def cut(self, frames, srs, widths):
        """Batches (lists of POSITIONS into the window) for clips with the given header fields.  Within a sample rate the
        clips that stage as int16 (mono PCM16, width 2) come before the ones that need the host decoder (width 4), so a
        batch mixes the two only at the seam; the byte cap is charged with what _stage really lays out (staged_bytes: a
        float clip in a rate group makes every clip of that group 4 bytes per sample).  ``bs`` / ``min_clips`` /
        ``min_tokens`` are lower bounds, ``byte_cap`` is the memory knob (page-locked host memory and HBM per batch in
        flight): --bs does not bound memory."""
        n = len(frames)
        if n == 0:
            return []
        order = np.lexsort((np.arange(n), frames, widths, srs))        # by rate, then int16-before-float, then length, then input order
        fr_l, sr_l, slow_l = frames.tolist(), srs.tolist(), (np.asarray(widths) != 2).tolist()      # (plain ints: the loop runs per item)

        def rate_cost(a, b):
            return 4 * (a + b) if b else 2 * a

        def cost(k, grp):
            # grp: rate -> (int16 frames, float frames) of the open batch -> (bytes clip k adds to it, the entry it leaves behind)
            sr, f = sr_l[k], fr_l[k]
            a, b = grp.get(sr, (0, 0))
            a2, b2 = (a, b + f) if slow_l[k] else (a + f, b)
            return rate_cost(a2, b2) - rate_cost(a, b), (sr, (a2, b2))
        return self._cut(frames, srs, order, cost, lambda pos: self.staged_bytes(frames, srs, widths, pos))

    def cut_raw(self, frames, srs, widths, fast, sizes=None):
        """cut for an Ingest that stages for the device decoder: ``widths`` are the bytes per frame each clip is STAGED with
        (block_align of a verbatim data chunk, 4 of a host-decoded entry) and a clip costs what raw_bytes says, whatever shares its
        group; ``fast`` (bool per clip) marks the mono PCM16 clips, which come first within a rate so that a group of them alone
        stays an int16 group.  ``sizes``: the staged bytes per clip where they are not frames x width (a FLAC frame region with its
        frame table)."""
        n = len(frames)
        if n == 0:
            return []
        order = np.lexsort((np.arange(n), frames, ~np.asarray(fast, dtype=bool), srs))
        size = (frames * widths if sizes is None else np.asarray(sizes, dtype=np.int64))
        size = (size + _RAW_ALIGN - 1) // _RAW_ALIGN * _RAW_ALIGN
        size_l = size.tolist()
        return self._cut(frames, srs, order, lambda k, grp: (size_l[k], None), lambda pos: int(size[np.asarray(pos, dtype=np.int64)].sum()))

    def _cut(self, frames, srs, order, cost, total_bytes):
        """The walk both cuts share.  cost(k, state of the open batch: a dict) -> (bytes clip k adds, (key, value) to record in the
        state or None); total_bytes(positions) -> the staged bytes of a would-be batch."""
        tokens = np.maximum(1, np.asarray(self.tokens_of(frames, srs), dtype=np.int64))
        out, cur, ct = [], [], 0
        grp, total = {}, 0
        need = max(self.bs, self.min_clips)
        cap, min_tokens = self.byte_cap, self.min_tokens
        sr_l, tk_l = srs.tolist(), tokens.tolist()
        for k in order.tolist():
            sr = sr_l[k]
            add, entry = cost(k, grp)
            if cur and (total + add > cap or sr != sr_l[cur[-1]] and len(cur) >= need):
                out.append(cur)
                cur, ct, grp, total = [], 0, {}, 0
                add, entry = cost(k, grp)
            cur.append(k)
            if entry is not None:
                grp[entry[0]] = entry[1]
            total += add
            ct += tk_l[k]
            if len(cur) >= need and ct >= min_tokens:
                out.append(cur)
                cur, ct, grp, total = [], 0, {}, 0
        if cur:
            out.append(cur)
        # a small remainder does not get a launch chain of its own when the batch before it can take it (the byte cap is a
        # staging-buffer size, soft by half): a BiLSTM launch over 7 long clips lasts as long as one over 128 of them
        if len(out) >= 2 and len(out[-1]) * 2 < need and srs[out[-1][0]] == srs[out[-2][-1]] \
                and total_bytes(out[-2] + out[-1]) <= self.byte_cap + self.byte_cap // 2:
            tail = out.pop()
            out[-1] = out[-1] + tail
        return out


class Ingest(object):
    """Iterate over staged batches of ``ds`` (a SpeechQualityDataset): ``for staged in Ingest(...)``; the caller
    turns ``staged.groups`` into H2D copies out of ``ring.buf[staged.slot]`` and reports the event behind them with
    ``ring.release_after``.  Batches are prepared ``depth`` ahead on a producer thread."""

    def __init__(self, ds, batches, pin, num_workers, depth=2, device=None, device_decode=False, device_flac=False):
        """``batches``: a list of index lists (staged exactly as given), or a LengthAware policy (the producer forms the
        batches itself from the headers).  ``device_decode``: a rate group that is not all mono PCM16 is staged as a 'raw' group
        (data chunks verbatim + a nisqa_wav_clip table, decoded by group_pcm on the GPU) instead of being decoded here.
        ``device_flac`` (with device_decode): a FLAC stream nisqa_ingest_flac_plan finds eligible is staged as its frame region
        and frame table and decoded by nisqa_flac_decode; without it FLAC files are decoded by the reader threads."""
        self.ds, self.batches = ds, batches
        self.device_decode = bool(device_decode)
        self.device_flac = bool(device_flac) and self.device_decode
        self.device = device
        self.ring = _take_ring(depth + 1, pin)
        # reader threads: what the caller asked for, but never more than the CPU budget leaves next to the producer and
        # consumer threads (over-subscribing a quota-limited container stalls the whole loop, see cpu_budget), and -- when
        # the producer pins itself and its native pool to the GPU's NUMA node -- never more than that node offers
        budget = cpu_budget()
        # one process per GPU (torchrun): the ranks of a node share its CPU quota
        try:
            local_world = max(1, int(os.environ.get('LOCAL_WORLD_SIZE', '1')))
        except ValueError:
            local_world = 1
        if local_world > 1:
            budget = max(2, budget // local_world)
        self.numa_cpus = set()
        if device is not None and os.environ.get('NISQA_INGEST_NUMA', '1') != '0':
            self.numa_cpus = gpu_local_cpus(device)
            if self.numa_cpus:
                budget = min(budget, len(self.numa_cpus))
        asked = int(num_workers or 0)
        if asked <= 0 and isinstance(batches, LengthAware):
            asked = budget                      # the reference's default (--num_workers 0): as many readers as the box allows
        # next to the readers run the producer and the consumer thread (mostly blocked in native calls / on events)
        self.workers = max(1, min(asked, budget - (3 if local_world == 1 else 1)))
        if asked > self.workers:
            _note_once('nisqa_amd.ingest: %d reader threads instead of the %d requested (CPU budget of this process: %d)'
                       % (self.workers, asked, budget))
        self.lib = _lib.load_ingest()
        # the filename column is read ONCE per loop (a pandas scalar lookup per item costs more host time than staging the
        # item's samples); not cached on the dataset: an in-place edit of the column between two calls must be seen
        self._col = ds.df[ds.filename_column].tolist() if hasattr(ds, 'df') and hasattr(ds, 'filename_column') else None
        self.q = queue.Queue(maxsize=depth)
        self.stop = threading.Event()
        self.stats = {'paths': 0.0, 'probe': 0.0, 'layout': 0.0, 'slot_wait': 0.0, 'read': 0.0, 'queue_wait': 0.0, 'batches': 0}
        self._helper = None                        # header-probe helper of _planned (joined in close)
        self.thread = threading.Thread(target=self._produce, name='nisqa-ingest', daemon=True)
        self.thread.start()

    # -- producer side ---------------------------------------------------------------------------------
    def _probe(self, idx, stats=None, chunk=None):
        """RIFF headers of items ``idx`` -> (names, encoded paths, header records as a numpy structured array).  stats: the
        dict the 'paths' / 'probe' seconds are added to (the helper thread of _planned passes its own: two threads never
        write self.stats).  chunk: headers per native call.  The native pool runs ONE job at a time (csrc/ingest.cpp: Pool::run), so a
        probe of 16 384 headers in one call keeps the readers that stage the batches in hand out of the pool for its whole 20 ms --
        the copy stream ran dry for 5-15 ms at every window boundary (rocprofv3 --memory-copy-trace); in chunks of 1 024 the reads
        wait 1.3 ms at most."""
        ds, L, n = self.ds, self.lib, len(idx)
        T, t0 = self.stats if stats is None else stats, time.perf_counter()
        if self._col is not None:                                  # the column as it was when this loop started
            col, d = self._col, ds.data_dir
            names = [os.path.join(d, col[i]) for i in idx]
        else:
            names = [ds.file_path(i) for i in idx]
        enc = [os.fsencode(p) for p in names]
        paths = (ctypes.c_char_p * n)(*enc)
        infos = (_lib.WavInfo * n)()
        t1 = time.perf_counter()
        T['paths'] += t1 - t0
        if chunk is None or n <= chunk:
            rc = L.nisqa_ingest_probe(paths, n, infos, self.workers)
        else:
            rc = 0
            for s in range(0, n, chunk):
                m = min(chunk, n - s)
                rc += L.nisqa_ingest_probe(ctypes.cast(ctypes.byref(paths, s * ctypes.sizeof(ctypes.c_char_p)), ctypes.POINTER(ctypes.c_char_p)),
                                           m, ctypes.cast(ctypes.byref(infos, s * ctypes.sizeof(_lib.WavInfo)), ctypes.POINTER(_lib.WavInfo)),
                                           self.workers)
        T['probe'] += time.perf_counter() - t1
        if rc:
            bad = next(k for k in range(n) if infos[k].status != _lib.WAV_OK)
            raise ValueError('Could not load file {}'.format(names[bad]))      # NISQA_lib.py:2305-2306
        info = np.ctypeslib.as_array(infos).copy()
        return names, enc, info, self._plan_flac(enc, info)

    def _plan_flac(self, enc, info):
        """nisqa_flac_plan records of the probed files (numpy structured array of lib.FlacPlan), or None when the device FLAC
        decoder is not asked for or no file is a FLAC stream (an all-WAV job plans nothing)."""
        if not self.device_flac:
            return None
        sel = np.flatnonzero(info['tag'] == _lib.WAV_TAG_FLAC)
        if len(sel) == 0:
            return None
        plans = np.zeros(len(info), dtype=FLAC_PLAN)
        sub_info = np.ascontiguousarray(info[sel])
        sub = np.zeros(len(sel), dtype=FLAC_PLAN)
        paths = (ctypes.c_char_p * len(sel))(*[enc[k] for k in sel.tolist()])
        for s0 in range(0, len(sel), 1024):                          # (in chunks: the native pool runs one job at a time, see _probe)
            m = min(1024, len(sel) - s0)
            rc = self.lib.nisqa_ingest_flac_plan(
                ctypes.cast(ctypes.byref(paths, s0 * ctypes.sizeof(ctypes.c_char_p)), ctypes.POINTER(ctypes.c_char_p)), m,
                ctypes.cast(sub_info.ctypes.data + s0 * sub_info.itemsize, ctypes.POINTER(_lib.WavInfo)),
                ctypes.cast(sub.ctypes.data + s0 * sub.itemsize, ctypes.POINTER(_lib.FlacPlan)), self.workers)
            if rc < 0:
                raise RuntimeError('nisqa_ingest_flac_plan failed')
        plans[sel] = sub
        return plans

    def _stage(self, idx, probed=None):
        """Stage one batch: layout from the headers, then every data chunk straight into a page-locked slot.  A FLAC stream whose
        frames the readers cannot index (nisqa_ingest_flac_read refuses it) sends the batch round again with that file on the host
        path: the host decoder then accepts it or raises the reference's error."""
        names, enc, info, plans = probed if probed is not None else self._probe(idx)
        info = np.ascontiguousarray(info)
        plans = None if plans is None else np.ascontiguousarray(plans).copy()
        while True:
            st = self._stage_once(idx, names, enc, info, plans)
            if st is not None:
                return st

    def _stage_once(self, idx, names, enc, info, plans):
        ds, L, n = self.ds, self.lib, len(idx)
        T = self.stats
        t2 = time.perf_counter()
        paths = (ctypes.c_char_p * n)(*enc)
        infos = ctypes.cast(info.ctypes.data, ctypes.POINTER(_lib.WavInfo))
        frames, srs = info['n_frames'], info['sample_rate']
        fast = _verbatim_i16(info)
        widths, verbatim = self._staged_widths(info) if self.device_decode else (None, None)
        dev_flac = np.zeros(n, dtype=bool) if plans is None else (plans['eligible'] != 0) & self._flac_takes(info)
        # batch layout from the headers alone: clips of one rate are contiguous, int16 if ALL of them are mono PCM16
        layout, total = [], 0
        dst_off = np.full(n, -1, dtype=np.int64)
        region_off, table_off = np.full(n, -1, dtype=np.int64), np.zeros(n, dtype=np.int64)
        clip_id = np.zeros(n, dtype=np.int32)
        for sr, sel in rate_groups(srs):
            is_i16 = bool(fast[sel].all())
            fl = dev_flac[sel]
            if fl.any():                                            # flac group: a raw group + frame regions + their frame rows
                size = np.where(fl, plans['region_bytes'][sel], frames[sel] * widths[sel])
                padded = (size + _RAW_ALIGN - 1) // _RAW_ALIGN * _RAW_ALIGN
                off = total + np.concatenate(([0], np.cumsum(padded[:-1])))
                rows = np.where(fl, plans['n_frames'][sel], 0).astype(np.int64)
                tab = total + int(padded.sum())
                nbytes = int(padded.sum()) + FLAC_FRAME.itemsize * int(rows.sum())
                dst_off[sel] = np.where(verbatim[sel] & ~fl, off, -1)
                region_off[sel] = np.where(fl, off, -1)
                table_off[sel] = tab + FLAC_FRAME.itemsize * (np.cumsum(rows) - rows)
                clip_id[sel] = np.cumsum(fl) - 1
                layout.append((int(sr), sel, 'flac', off, nbytes))
                total = (total + nbytes + _ALIGN - 1) // _ALIGN * _ALIGN
                continue
            if self.device_decode and not is_i16:                   # raw group: every clip at its own width, on a 16-byte boundary
                size = frames[sel] * widths[sel]
                padded = (size + _RAW_ALIGN - 1) // _RAW_ALIGN * _RAW_ALIGN      # (the last clip's pad is the tail pad of the group)
                off = total + np.concatenate(([0], np.cumsum(padded[:-1])))
                nbytes = int(padded.sum())
                dst_off[sel] = np.where(verbatim[sel], off, -1)
                layout.append((int(sr), sel, 'raw', off, nbytes))
                total = (total + nbytes + _ALIGN - 1) // _ALIGN * _ALIGN
                continue
            width = 2 if is_i16 else 4
            off = total + np.concatenate(([0], np.cumsum(frames[sel][:-1]))) * width
            nbytes = int(frames[sel].sum()) * width
            if is_i16:
                dst_off[sel] = off
            layout.append((int(sr), sel, 'i16' if is_i16 else 'f32', off, nbytes))
            total = (total + nbytes + _ALIGN - 1) // _ALIGN * _ALIGN
        t3 = time.perf_counter()
        T['layout'] += t3 - t2
        slot = self.ring.acquire(max(total, _ALIGN))
        buf = self.ring.buf[slot]
        t4 = time.perf_counter()
        T['slot_wait'] += t4 - t3
        rc = L.nisqa_ingest_read(paths, n, infos, ctypes.c_void_p(buf.data_ptr()),
                                 dst_off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), self.workers)
        if dev_flac.any() and not rc:
            status = np.zeros(n, dtype=np.int32)
            bad = L.nisqa_ingest_flac_read(paths, n, ctypes.cast(plans.ctypes.data, ctypes.POINTER(_lib.FlacPlan)),
                                           ctypes.c_void_p(buf.data_ptr()), region_off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                           table_off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                           clip_id.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                           status.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), self.workers)
            if bad:                                                 # these files take the host path: lay the batch out again
                T['read'] += time.perf_counter() - t4
                self.ring.release_after(slot, None)
                if bad < 0:
                    raise RuntimeError('nisqa_ingest_flac_read failed')
                plans['eligible'][status != 0] = 0
                return None
        T['read'] += time.perf_counter() - t4
        T['batches'] += 1
        if rc:
            bad = next(k for k in range(n) if info['status'][k] != _lib.WAV_OK)
            self.ring.release_after(slot, None)
            raise ValueError('Could not load file {}'.format(names[bad]))
        groups = []
        raw = None
        for sr, sel, kind, off, nbytes in layout:
            clips = flac = None
            if kind != 'i16':                                       # stereo / 8, 24, 32-bit / float: host decode ...
                raw = buf.numpy() if raw is None else raw
                for k, o in zip(sel.tolist(), off.tolist()):
                    if dst_off[k] >= 0 or region_off[k] >= 0:       # ... unless the data chunk / frame region went in verbatim
                        continue
                    y, _ = wavio.read_wav(names[k], ds.ms_channel)
                    if y.dtype == np.int16:
                        y = y.astype(np.float32) / np.float32(32768.0)
                    raw[o:o + 4 * len(y)].view(np.float32)[:] = y
            if kind == 'raw':
                clips = self._clip_table(info[sel], verbatim[sel], off - int(off[0]))
            elif kind == 'flac':
                fl = dev_flac[sel]
                dst = np.concatenate(([0], np.cumsum(frames[sel][:-1])))
                clips = self._clip_table(info[sel], verbatim[sel], off - int(off[0]))[~fl]
                flac = {'clips': self._flac_table(plans[sel][fl], (off - int(off[0]))[fl], dst[fl]), 'pos': np.flatnonzero(fl),
                        'frames_off': int(table_off[sel][0]) - int(off[0]), 'n_rows': int(plans['n_frames'][sel][fl].sum()),
                        'as_i16': bool(fast[sel].all())}
            groups.append(Group([idx[k] for k in sel.tolist()], frames[sel].tolist(), sr, int(off[0]) if len(off) else 0,
                                nbytes, kind == 'i16', [names[k] for k in sel.tolist()], kind, clips, flac))
        return Staged(slot, groups)

    def _flac_takes(self, info):
        """Which FLAC files the device decoder can serve for this dataset: an ms_channel the stream does not have stays with the host
        decoder, which raises the reference's error for it."""
        sel = getattr(self.ds, 'ms_channel', None)
        ch = info['channels']
        return (info['tag'] == _lib.WAV_TAG_FLAC) & ((ch == 1) | (ch == 2) & (True if sel is None else (0 <= int(sel) < 2)))

    def _flac_table(self, plans, src_off, dst_off):
        """nisqa_flac_clip rows of a flac group's device-decoded streams (frame0 and md5_off are the engine's)."""
        t = np.zeros(len(plans), dtype=FLAC_CLIP)
        sel = getattr(self.ds, 'ms_channel', None)
        t['src_off'], t['src_bytes'], t['dst_off'], t['n_samples'] = src_off, plans['region_bytes'], dst_off, plans['n_samples']
        for f in ('n_frames', 'block_size', 'bits', 'channels', 'md5_set', 'md5'):
            t[f] = plans[f]
        t['channel'] = -1 if sel is None else np.where(plans['channels'] > 1, int(sel), 0)
        return t

    def _staged_widths(self, info):
        """Device decode: (bytes per frame each file is staged with, which files nisqa_ingest_read puts into the slot itself).  A WAV
        file nisqa_wav_decode takes goes in verbatim at block_align bytes per frame, a mono 16-bit FLAC stream is decoded into the
        slot as int16 by the reader threads; what is left -- other FLAC streams, a mean over more than 32 channels, a frame wider
        than the kernel stages, an ms_channel the file does not have (the host decoder raises the reference's error for it) -- is
        decoded on the host into float32."""
        ch, blk = info['channels'].astype(np.int64), info['block_align'].astype(np.int64)
        flac = info['tag'] == _lib.WAV_TAG_FLAC
        sel = getattr(self.ds, 'ms_channel', None)
        one = (ch == 1) | ((ch <= _lib.WAV_DECODE_MAX_MEAN) if sel is None else (ch > int(sel)) & (int(sel) >= 0))
        wav = ~flac & one & (blk <= _lib.WAV_DECODE_MAX_BLOCK)
        flac16 = flac & (info['bits'] == 16) & (ch == 1)
        return np.where(wav, blk, np.where(flac16, 2, 4)), wav | flac16

    def _clip_table(self, info, verbatim, src_off):
        """nisqa_wav_clip rows of a raw group's files (header records ``info``, byte offsets ``src_off`` from the group's start)."""
        t = np.zeros(len(info), dtype=WAV_CLIP)
        ch = info['channels']
        wav = verbatim & (info['tag'] != _lib.WAV_TAG_FLAC)
        sel = getattr(self.ds, 'ms_channel', None)
        t['src_off'] = src_off
        t['dst_off'] = np.concatenate(([0], np.cumsum(info['n_frames'][:-1])))
        t['n_frames'] = info['n_frames']
        t['channels'] = np.where(wav, ch, 1)
        t['container'] = np.where(wav, info['block_align'] // np.maximum(ch, 1), np.where(verbatim, 2, 4))
        # a mono 16-bit FLAC stream lies in its slot as mono PCM16, a host-decoded file as mono little-endian float32
        t['encoding'] = np.where(wav, info['tag'], np.where(verbatim, _lib.WAVENC_PCM, _lib.WAVENC_FLOAT))
        t['channel'] = -1 if sel is None else np.where(wav & (ch > 1), int(sel), 0)
        return t

    def _planned(self):
        """Batches of a LengthAware policy: yields (idx, probed) window by window; the headers of window w + 1 are
        probed on a helper thread while the batches of window w are staged."""
        pol = self.batches
        # the FIRST window is small: its probe and cut run before anything is staged (25-35 ms for 16 384 headers -- 1.5 % of a
        # 100 000-row job during which the link carries nothing); every later window is prepared under the one before it
        first = min(pol.window, 2048)
        starts = [0] + list(range(first, len(pol.indices), pol.window)) if len(pol.indices) > first else [0]
        wins = [pol.indices[s:e] for s, e in zip(starts, starts[1:] + [len(pol.indices)])] if len(pol.indices) else []
        box = {}

        def probe_into(w):
            # runs on the helper thread: timings stay local and are merged by the producer; a loop that was closed
            # (self.stop) probes nothing more
            loc = {'paths': 0.0, 'probe': 0.0}
            try:
                if self.stop.is_set():
                    box[w] = ('stop', None, loc)
                    return
                names, enc, info, plans = self._probe(wins[w], loc, chunk=None if w == 0 else 1024)    # (w >= 1: in the background, under window w - 1's staging)
                # the window's batches are cut HERE, on the helper thread: sorting and walking 16 384 items in Python is
                # 10-20 ms during which the producer staged nothing and the link ran dry once per window
                fast = _verbatim_i16(info)
                if self.device_decode:                                  # the byte cap is charged with the staged widths
                    sizes = None
                    if plans is not None:                               # (a frame region with its frame rows: what is staged for it)
                        dev = (plans['eligible'] != 0) & self._flac_takes(info)
                        sizes = np.where(dev, plans['region_bytes'] + FLAC_FRAME.itemsize * plans['n_frames'].astype(np.int64),
                                         info['n_frames'].astype(np.int64) * self._staged_widths(info)[0])
                    cuts = pol.cut_raw(info['n_frames'].astype(np.int64), info['sample_rate'].astype(np.int64),
                                       self._staged_widths(info)[0], fast, sizes)
                else:
                    cuts = pol.cut(info['n_frames'].astype(np.int64), info['sample_rate'].astype(np.int64), np.where(fast, 2, 4))
                box[w] = ('ok', (names, enc, info, cuts, plans), loc)
            except BaseException as e:
                box[w] = ('err', e, loc)

        helper = None
        if wins:
            probe_into(0)
        for w in range(len(wins)):
            if helper is not None:
                helper.join()
                self._helper = None
            kind, val, loc = box.pop(w)
            for k_, v_ in loc.items():
                self.stats[k_] += v_
            if kind == 'stop':
                return
            if kind == 'err':
                raise val
            if w + 1 < len(wins):
                helper = self._helper = threading.Thread(target=probe_into, args=(w + 1,), name='nisqa-probe', daemon=True)
                helper.start()
            else:
                helper = None
            names, enc, info, cuts, plans = val
            for pos in cuts:
                yield [wins[w][k] for k in pos], ([names[k] for k in pos], [enc[k] for k in pos], info[pos], None if plans is None else plans[pos])

    def _produce(self):
        try:
            if self.numa_cpus:
                try:                                       # this thread only; the native reader pool inherits it
                    os.sched_setaffinity(0, self.numa_cpus)
                except OSError:
                    pass
            it = self._planned() if isinstance(self.batches, LengthAware) else ((idx, None) for idx in self.batches)
            for idx, probed in it:
                if self.stop.is_set():
                    return
                st = self._stage(idx, probed)
                t0 = time.perf_counter()
                self.q.put(('ok', st))
                self.stats['queue_wait'] += time.perf_counter() - t0
            self.q.put(('end', None))
        except BaseException as e:             # surfaces in the consumer, like a DataLoader worker error
            self.q.put(('err', e))

    # -- consumer side ---------------------------------------------------------------------------------
    def __iter__(self):
        while True:
            kind, val = self.q.get()
            if kind == 'end':
                return
            if kind == 'err':
                raise val
            yield val

    def close(self, keep_ring=True):
        """keep_ring=False: the page-locked ring is freed instead of being kept for the next loop."""
        if self.ring is None:                      # already closed
            return
        self.stop.set()
        self.ring.abandon()
        try:
            while True:                        # unblock a producer waiting on a full queue
                self.q.get_nowait()
        except queue.Empty:
            pass
        self.thread.join(timeout=30)
        helper = self._helper
        if helper is not None:                     # a probe of the next window still running: it sees self.stop, or finishes
            helper.join(timeout=30)
        if keep_ring and not self.thread.is_alive():
            _give_ring(self.ring)                  # the consumer's release events are still attached: reset() waits for them
        self.ring = None


# -- what both loops do with a staged group ------------------------------------------------------------------
def device_decode_default():
    """Whether the predict and the training loop stage for the device decoder: yes, unless NISQA_HOST_DECODE=1 asks for the
    host-decoding Ingest (the A/B switch and the cross-check of nisqa_wav_decode)."""
    return os.environ.get('NISQA_HOST_DECODE') != '1'


def device_flac_default():
    """Whether the loops also stage FLAC streams for the device decoder (nisqa_flac_decode): yes, unless NISQA_HOST_FLAC=1 (the
    reader threads decode FLAC, as before: the A/B switch and the cross-check) or NISQA_HOST_DECODE=1 asks for host decoding
    altogether."""
    return os.environ.get('NISQA_HOST_FLAC') != '1' and device_decode_default()


def copy_group(buf, g, device):
    """H2D copy of group ``g`` out of the ring buffer ``buf`` (on the current stream): int16 / float32 samples, or the bytes of a raw
    or flac group."""
    host = buf[g.offset:g.offset + g.nbytes]
    if g.kind not in ('raw', 'flac'):
        host = host.view(torch.int16 if g.kind == 'i16' else torch.float32)
    return host.to(device, non_blocking=True)


def decode_group(x, g, eng):
    """The device PCM of group ``g`` from what copy_group sent (on the current stream): int16 and float32 groups as they are, a raw
    group through nisqa_wav_decode -> float32 [sum of lengths]."""
    if g.kind == 'flac':
        f, total = g.flac, int(sum(g.lengths))
        if f['as_i16']:                                              # every clip mono 16-bit: the int16 entry's form
            out = torch.empty(total, dtype=torch.int16, device=x.device)
            for row in g.clips:                                      # (mono PCM16 data chunks next to the streams: in place)
                a, d, m = int(row['src_off']), int(row['dst_off']), int(row['n_frames'])
                out[d:d + m].copy_(x[a:a + 2 * m].view(torch.int16))
        else:
            out = torch.empty(total, dtype=torch.float32, device=x.device)
            if len(g.clips):
                eng.decode(x, g.clips, total, out=out)
        out, g.status = eng.flac_decode(x, f['clips'], f['frames_off'], f['n_rows'], total, f['as_i16'], out=out)
        return out
    if g.kind != 'raw':
        return x
    return eng.decode(x, g.clips, int(sum(g.lengths)))


def check_flac_status(g, status, ms_channel=None):
    """The status words nisqa_flac_decode left for group ``g`` (host array, [clips + 1]): nothing when all are zero.  For a flagged
    stream the host decoder is asked: if it refuses the file too this is the reference's unreadable file; if it accepts, the device
    decoder misread a stream or the frame index hit a false sync -- an error either way, never different audio."""
    if g.kind != 'flac' or status is None:
        return
    status = np.asarray(status).reshape(-1)
    if not status.any():
        return
    if status[-1]:
        raise RuntimeError('nisqa_flac_decode: a frame table row names no clip (status 0x%x)' % int(status[-1]))
    k = int(np.flatnonzero(status)[0])
    name = g.names[int(g.flac['pos'][k])]
    try:
        wavio.read_wav(name, ms_channel)
    except Exception:
        raise ValueError('Could not load file {}'.format(name))      # NISQA_lib.py:2305-2306
    raise RuntimeError('nisqa_flac_decode refused {} (status 0x{:x}) but the host decoder reads it: a decoder bug or a false frame '
                       'sync; NISQA_HOST_FLAC=1 decodes FLAC on the host'.format(name, int(status[k])))


def group_pcm(buf, g, eng, ms_channel=None):
    """(ring buffer, Group, engine) -> the group's PCM on the engine's device: int16 for an 'i16' group, float32 for an 'f32' group,
    copy + decode for a 'raw' one.  (A loop that copies and computes on different streams calls the two halves itself.)"""
    out = decode_group(copy_group(buf, g, eng.device), g, eng)
    if g.kind == 'flac':                                             # (this convenience form waits for the words; the predict loop does not)
        check_flac_status(g, g.status.cpu().numpy(), ms_channel)
    return out
