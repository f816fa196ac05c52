"""Support of the audio-gradient tests (not a test module): a torch restatement of the mel front end as a differentiable function of
the samples, the segment indexing behind it, its composition with the float64 network oracles, and the seeded test signals.

The six steps, per clip: reflect pad by n_fft / 2, frames of n_fft samples every hop, the periodic hann window of
oracle.mel.hann_periodic centred in the frame, torch.fft.rfft, the float32 weights of oracle.mel.mel_filterbank applied to |X|,
db = 10 log10(max(1e-8, M^2)), out = max(db, max(db) - 80).  In float64 this is the reference the kernels of csrc/mel_bwd.hip are
held to; evaluated in float32 on the CPU it shows what that width alone costs.

MARGIN of an evaluation: the smallest distance in dB of any element to the clip's floor or to the amin threshold (-80 dB), and the
gap between the two largest elements of the clip.  Above 1e-2 dB -- ten times the project's 1e-3 dB mel parity bar -- an fp32
evaluation cannot sit on the other side of a gate or choose another maximum, so nothing needs to be left out of a comparison.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import mel as omel

N_FFT, N_MELS, AMIN_SQ, TOP_DB = 4096, 48, 1e-8, 80.0
MARGIN_DB = 1e-2
RATES = (48000, 16000, 22050, 96000)


def fmax_of(sr):
    return float(min(20000, sr // 2))


def hop_win(sr):
    return int(sr * 0.01), int(sr * 0.02)                      # NISQA_lib.py:2308-2309


def mel_forward(y, sr, fmax=None, dtype=torch.float64):
    """y: 1-D tensor of samples -> (clamped dB rows [T, 48], unclamped dB rows [T, 48], margin in dB, gap of the two largest
    elements in dB), all in ``dtype``; differentiable in y."""
    hop, win = hop_win(sr)
    fmax = fmax_of(sr) if fmax is None else float(fmax)
    y = y.to(dtype)
    w = torch.zeros(N_FFT, dtype=dtype)
    lpad = (N_FFT - win) // 2
    w[lpad:lpad + win] = torch.from_numpy(omel.hann_periodic(win)).to(dtype)
    fb = torch.from_numpy(omel.mel_filterbank(sr, N_FFT, N_MELS, 0.0, fmax)).to(dtype)       # float32 weights, as librosa's
    ypad = F.pad(y[None, None], (N_FFT // 2, N_FFT // 2), mode='reflect')[0, 0]
    frames = ypad.unfold(0, N_FFT, hop)                         # [T, 4096], T = 1 + len(y) // hop
    mag = torch.fft.rfft(frames * w, dim=1).abs()
    m = mag @ fb.t()
    p = m * m
    db = 10.0 * torch.log10(torch.clamp(p, min=AMIN_SQ))
    floor = db.max() - TOP_DB
    out = torch.maximum(db, floor)
    with torch.no_grad():
        raw = 10.0 * torch.log10(torch.clamp(p, min=1e-300))     # the power itself in dB: its distance to amin
        margin = float(torch.minimum((db - floor).abs().min(), (raw - 10.0 * np.log10(AMIN_SQ)).abs().min()))
        top = db.flatten().topk(2)[0]
        gap = float(top[0] - top[1])
    return out, db, margin, gap


def mel_vjp(y, sr, g, fmax=None, dtype=torch.float64):
    """d (sum g * clamped dB rows) / d y for one clip: y [L], g [T, 48] -> (dy [L], out, db, margin, gap) as numpy / floats"""
    yt = torch.as_tensor(np.asarray(y)).to(dtype).clone().requires_grad_(True)
    out, db, margin, gap = mel_forward(yt, sr, fmax, dtype)
    dy, = torch.autograd.grad((out * torch.as_tensor(np.asarray(g)).to(dtype)).sum(), yt)
    return dy.numpy(), out.detach().numpy(), db.detach().numpy(), margin, gap


def regimes(db, out_floor_g):
    """db [T, 48] unclamped rows of one clip (float64), g the gradient on the clamped rows -> (elements clamped by the floor
    alone that carry a non-zero g, elements under amin)"""
    floor = db.max() - TOP_DB
    under = db <= 10.0 * np.log10(AMIN_SQ)
    return int(((db < floor) & ~under & (out_floor_g != 0)).sum()), int(under.sum())


def segment_index(T, seg_hop, seg_len=15):
    """frames of the segments of a T-frame clip: [n_wins, seg_len] (NISQA_lib.py:2256, 2266-2280)"""
    n_full = T - (seg_len - 1)
    n_wins = -(-n_full // seg_hop) if seg_hop > 1 else n_full
    return seg_hop * np.arange(n_wins)[:, None] + np.arange(seg_len)[None, :]


def segments_of(rows, seg_hop):
    """clamped rows [T, 48] (numpy or tensor) -> x [n_wins, 1, 48, 15]: oracle.net.segment_specs's indexing on time-major rows"""
    idx = segment_index(rows.shape[0], seg_hop)
    x = rows[idx]                                                # [n_wins, 15, 48]
    return (x.permute(0, 2, 1) if torch.is_tensor(x) else np.transpose(x, (0, 2, 1)))[:, None]


def segments_adjoint(dx, T, seg_hop):
    """dx [n_wins, 1, 48, 15] float64 -> d / d rows [T, 48]: index_add over the segments"""
    idx = torch.from_numpy(segment_index(T, seg_hop))
    d = torch.zeros((T, N_MELS), dtype=torch.float64)
    src = torch.as_tensor(np.asarray(dx), dtype=torch.float64)[:, 0].permute(0, 2, 1)        # [n_wins, 15, 48]
    d.index_add_(0, idx.reshape(-1), src.reshape(-1, N_MELS))
    return d.numpy()


def compose(net_oracle, sd, args, rows, ys, sr, gs, L=None):
    """The wanted d (sum g * model) / d y of a batch: ``rows`` the clamped dB rows [T_b, 48] per clip AS THE ENGINE COMPUTED THEM
    (float32), ys the samples per clip, gs a list of g [B, heads].  The float64 network gradient (net_oracle: input_grad_oracle.oracle
    or input_grad_lstm_oracle.oracle) is evaluated at the segment tensor cut from those rows -- so the ReLU and max-pool choices
    are compared at one point -- and pulled back through the float64 restatement's vector-Jacobian product at y.
    -> dict(dy: per g a list of [L_b] arrays, y [B, heads], margin [B, L] the network's tie margins, mel_margin, mel_gap per clip)"""
    seg_hop = args['ms_seg_hop_length']
    segs = [segments_of(np.asarray(r, dtype=np.float32), seg_hop) for r in rows]
    n_wins = np.array([len(s) for s in segs], dtype=np.int64)
    L = int(n_wins.max()) if L is None else L
    x = np.zeros((len(rows), L, 1, 48, 15), dtype=np.float32)
    for b, s in enumerate(segs):
        x[b, :len(s)] = s
    net = net_oracle(sd, args, x, n_wins, gs)
    dy, mm, mg = [[] for _ in gs], [], []
    for b, yb in enumerate(ys):
        T = rows[b].shape[0]
        for k in range(len(gs)):
            grow = segments_adjoint(net['dx'][k][b, :n_wins[b]], T, seg_hop)
            d, _, _, margin, gap = mel_vjp(yb, sr, grow, args['ms_fmax'])
            dy[k].append(d)
        mm.append(margin)
        mg.append(gap)
    return {'dy': dy, 'y': net['y'], 'margin': net['margin'], 'mel_margin': np.array(mm), 'mel_gap': np.array(mg), 'n_wins': n_wins,
            'x': x}


# ---- the seeded signals ---------------------------------------------------------------------------------------------------------
FRAMES = (15, 23, 19)


def lengths_of(sr, frames=FRAMES):
    """(T - 1) hop + r with r = 0, an odd remainder, hop - 1: every way a clip can end inside its last hop"""
    hop = hop_win(sr)[0]
    odd = (hop // 3) | 1
    return [(T - 1) * hop + r for T, r in zip(frames, (0, odd, hop - 1))]


def gate_signal(sr, n, seed):
    """n samples in three stretches: LOUD (two tones under a rising-falling envelope that peaks near full scale, over broadband
    noise: one largest element, every band alive), exact ZEROS for 2.25 windows (whole frames are silent: every band under
    amin), and QUIET noise whose bands land between amin (-80 dB) and the clip's floor (max - 80 dB): clamped by the floor alone.
    The quiet level is set from the loud part's own maximum: half way (in dB) between amin and the floor it implies."""
    rng = np.random.default_rng(seed)
    hop, win = hop_win(sr)
    n_zero = 2 * win + win // 4
    n_quiet = max(2 * win, (n - n_zero) // 3)
    n_loud = n - n_zero - n_quiet
    assert n_loud >= 2 * win
    t = np.arange(n_loud) / float(sr)
    env = np.sin(np.pi * (np.arange(n_loud) + 0.37 * hop) / (n_loud + 0.9 * hop)) ** 2
    loud = env * (0.55 * np.sin(2 * np.pi * rng.uniform(350, 500) * t + rng.uniform(0, 6))
                  + 0.3 * np.sin(2 * np.pi * rng.uniform(1300, 1700) * t + rng.uniform(0, 6))) + 0.12 * rng.uniform(-1, 1, n_loud)
    y = np.zeros(n, dtype=np.float32)
    y[:n_loud] = loud.astype(np.float32)
    noise = rng.standard_normal(n_quiet)
    # the level of unit noise in its own frames, then scaled to sit between -80 dB and the floor of the loud part
    with torch.no_grad():
        top = float(mel_forward(torch.from_numpy(y.astype(np.float64)), sr)[1].max())            # (the rest is still zero)
        ref = float(mel_forward(torch.from_numpy(rng.standard_normal(3 * N_FFT)), sr)[1].median())
    assert top - TOP_DB > -TOP_DB + 6.0, 'the loud part must lift the floor clear of amin'
    target = 0.5 * ((top - TOP_DB) + (-TOP_DB))
    y[n - n_quiet:] = (noise * 10.0 ** ((target - ref) / 20.0)).astype(np.float32)
    return y


# (rate, clip) -> seed of gate_signal: the first seeds whose float64 evaluation has all three regimes and a margin >= MARGIN_DB
GATE_SEEDS = {(sr, b): 100 * b + 1 for sr in RATES for b in range(3)}
GATE_SEEDS[(22050, 2)] = 202                  # (seed 201 leaves an element 0.005 dB from the floor)


def gate_batch(sr):
    """the three clips of a rate: (list of float32 sample arrays, lengths)"""
    lengths = lengths_of(sr)
    return [gate_signal(sr, n, GATE_SEEDS[(sr, b)]) for b, n in enumerate(lengths)], lengths


def smooth_signal(sr, n, seed):
    """n samples of broadband noise under a slow envelope with two tones: every band well above the floor and amin (nothing is
    clamped, so no two pixels of the network's input are equal): the end-to-end signals."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / float(sr)
    env = 0.35 + 0.3 * np.sin(2 * np.pi * rng.uniform(3, 9) * t + rng.uniform(0, 6))
    y = env * (0.5 * rng.standard_normal(n) + 0.4 * np.sin(2 * np.pi * rng.uniform(200, 900) * t)
               + 0.3 * np.sin(2 * np.pi * rng.uniform(2000, 6000) * t))
    return np.clip(y, -1, 1).astype(np.float32)


def clip_errors(got, want):
    """max |got - want| / max |want| per clip, for lists of per-clip arrays"""
    return np.array([np.abs(np.asarray(g, dtype=np.float64) - w).max() / np.abs(w).max() for g, w in zip(got, want)])
