"""The project's own statement of the FARGAN training losses, in torch on the
CPU, with the dtype as a parameter: float64 is the yardstick of the GPU tests,
float32 the comparison point their gates are held against.

Written from the formulas, not from the reference's code:
  s = sqrt(max(|STFT(x)|, 1e-7)), STFT centred with reflect padding, a window
  of win_length zero-padded to fft_size ((fft_size - win_length) // 2 left);
  spectral convergence = sum |s_y - s_x| / sum s_y over the whole batch;
  G = d (sum |s_y - s_x|) / d X = -sign(s_y - s_x) X / (2 s_x |X|) where |X| >
  1e-7, 0 elsewhere (as Re + i Im, torch's convention for a complex gradient);
  signal = mean over rows of 1 - <p, t>, p and t the rows over (1e-15 + norm).
"""
import math

import torch

FLOOR = 1e-7
DEFAULT_RESOLUTIONS = tuple(
    (n, n // 4, n) for n in (2560, 1280, 640, 320, 160, 80))


def window_table(name, win_length, fft_size, dtype=torch.float64):
    """getattr(torch, name)(win_length) centred in fft_size zeros"""
    window = getattr(torch, name)(win_length, dtype=torch.float64)
    left = (fft_size - win_length) // 2
    table = torch.zeros(fft_size, dtype=torch.float64)
    table[left:left + win_length] = window
    return table.to(dtype)


def framed(x, fft_size, hop_size):
    """(B, T) -> (B, frames, fft_size): reflect padding of fft_size / 2,
    frames = 1 + T // hop_size"""
    half = fft_size // 2
    padded = torch.nn.functional.pad(x[:, None], (half, half), 'reflect')[:, 0]
    return padded.unfold(-1, fft_size, hop_size)


def transform(x, fft_size, hop_size, win_length, window='hann_window'):
    """One-sided STFT (B, fft_size / 2 + 1, frames), complex, in x's dtype"""
    table = window_table(window, win_length, fft_size, x.dtype)
    frames = framed(x, fft_size, hop_size) * table
    return torch.fft.rfft(frames, dim=-1).transpose(1, 2)


def magnitude_root(X):
    return torch.sqrt(torch.clamp(X.abs(), min=FLOOR))


def stft(x, fft_size, hop_size, win_length, window='hann_window'):
    return magnitude_root(transform(x, fft_size, hop_size, win_length, window))


def spectral_convergence(x, y, fft_size, hop_size, win_length,
                         window='hann_window'):
    s_x = stft(x, fft_size, hop_size, win_length, window)
    s_y = stft(y, fft_size, hop_size, win_length, window)
    return (s_y - s_x).abs().sum() / s_y.sum()


def multi_resolution(x, y, resolutions=DEFAULT_RESOLUTIONS,
                     window='hann_window'):
    losses = [spectral_convergence(x, y, *r, window) for r in resolutions]
    return sum(losses) / len(losses)


def signal(y_true, y_pred):
    t = y_true / (1e-15 + y_true.norm(dim=-1, keepdim=True))
    p = y_pred / (1e-15 + y_pred.norm(dim=-1, keepdim=True))
    return (1. - (p * t).sum(-1)).mean()


###############################################################################
# Hand-written derivatives (checked against autograd in test_cpu_losses.py)
###############################################################################


def bin_gradient(x, y, fft_size, hop_size, win_length, window='hann_window'):
    """G = d sum |s_y - s_x| / d X, complex (B, bins, frames)"""
    X = transform(x, fft_size, hop_size, win_length, window)
    s_x = magnitude_root(X)
    s_y = stft(y, fft_size, hop_size, win_length, window)
    magnitude = X.abs()
    live = magnitude > FLOOR
    factor = -torch.sign(s_y - s_x) * .5 / (s_x * magnitude.clamp(min=FLOOR))
    return torch.where(live, factor * X, torch.zeros_like(X))


def adjoint(G, samples, fft_size, hop_size, win_length,
            window='hann_window'):
    """The adjoint of x -> transform(x) applied to G (B, bins, frames):
    d <G, STFT(x)> / d x with <a, b> = sum Re a Re b + Im a Im b."""
    real = G.real.dtype
    table = window_table(window, win_length, fft_size, real)
    batch, bins, frames = G.shape
    # every bin once: irfft doubles the interior bins, so halve them first
    weights = torch.full((bins, 1), .5, dtype=real)
    weights[0] = weights[-1] = 1.
    u = torch.fft.irfft(
        (G * weights).transpose(1, 2), n=fft_size, dim=-1, norm='forward')
    u = u * table
    half = fft_size // 2
    padded = torch.zeros(batch, samples + fft_size, dtype=real)
    for f in range(frames):
        padded[:, f * hop_size:f * hop_size + fft_size] += u[:, f]
    out = padded[:, half:half + samples].clone()
    # reflect: padded sample half - i is sample i (1 <= i <= half) and padded
    # sample half + 2 (T - 1) - i is sample i (T - 1 - half <= i <= T - 2)
    out[:, 1:half + 1] += padded[:, :half].flip(-1)
    out[:, samples - 1 - half:samples - 1] += padded[:, half + samples:].flip(-1)
    return out


def signal_gradient(y_true, y_pred):
    rows = y_pred[..., 0].numel()
    norm_t = 1e-15 + y_true.norm(dim=-1, keepdim=True)
    norm = y_pred.norm(dim=-1, keepdim=True)
    norm_p = 1e-15 + norm
    dot = (y_pred * y_true).sum(-1, keepdim=True)
    first = y_true / (norm_t * norm_p)
    second = dot * y_pred / (norm_t * norm.clamp(min=1e-300) * norm_p ** 2)
    second = torch.where(norm > 0, second, torch.zeros_like(second))
    return -(first - second) / rows


###############################################################################
# Error model of an fp32 transform (the gates of test_gpu_losses.py)
###############################################################################


def delta(x, fft_size, hop_size, win_length, window='hann_window'):
    """2^-24 log2(N) |windowed frame|_2 per frame, (B, 1, frames), float64"""
    x = x.double()
    table = window_table(window, win_length, fft_size)
    frames = framed(x, fft_size, hop_size) * table
    return (2. ** -24 * math.log2(fft_size) * frames.norm(dim=-1))[:, None]


def fragile(x, y, fft_size, hop_size, win_length, window='hann_window'):
    """Bins where fp32 rounding may flip the sign of s_y - s_x or the phase of
    X: bool (B, bins, frames)"""
    x, y = x.double(), y.double()
    X = transform(x, fft_size, hop_size, win_length, window)
    Y = transform(y, fft_size, hop_size, win_length, window)
    s_x, s_y = magnitude_root(X), magnitude_root(Y)
    d_x = delta(x, fft_size, hop_size, win_length, window)
    d_y = delta(y, fft_size, hop_size, win_length, window)
    return (((s_y - s_x).abs() <= 64 * (d_x / (2 * s_x) + d_y / (2 * s_y)))
            | (X.abs() <= 64 * d_x) | (Y.abs() <= 64 * d_y))


def inputs(seed, batch, samples, sigma=.1):
    """The seeded Gaussian inputs the tests share: x, y (batch, samples) fp32"""
    generator = torch.Generator().manual_seed(seed)
    x = sigma * torch.randn(batch, samples, generator=generator)
    y = sigma * torch.randn(batch, samples, generator=generator)
    return x, y


###############################################################################
# The cases test_gpu_losses.py runs (test_cpu_losses.py checks their inputs)
###############################################################################

CONFIGURATIONS = DEFAULT_RESOLUTIONS + (
    (1024, 120, 600), (64, 16, 64), (2048, 512, 2048))
SHAPES = ((3, 4096), (1, 4099), (2, 1281))          # (batch, samples)
NOISE_SEED = 7
SCALES = (2., .5, 2.)                               # y = c_b x, end to end


def shapes_of(fft_size):
    """The shapes a configuration runs on: those long enough for its reflect
    padding, and for the small sizes the shortest row it admits."""
    shapes = [s for s in SHAPES if s[1] > fft_size // 2]
    if fft_size <= 160:
        shapes.append((2, fft_size // 2 + 1))
    return shapes


def scaled_inputs(seed, batch, samples):
    """x and y = c_b x: both signs of s_y - s_x, no ties"""
    x, _ = inputs(seed, batch, samples)
    return x, x * torch.tensor(SCALES[:batch])[:, None]


# (no bin of any default resolution is fragile on scaled_inputs(END_TO_END_SEED,
# ...) at any of SHAPES: test_cpu_losses.py asserts it)
END_TO_END_SEED = 100
