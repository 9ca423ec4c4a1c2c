"""Mel spectrogram reconstruction: drop-in for `promonet.baseline.mels`
(promonet/baseline/mels.py), run under config/baselines/vocos.py
(MODEL = 'vocos', SPECTROGRAM_ONLY = True).

Audio -> spectrogram (pm_stft_magnitude) -> MelGenerator (linear_to_mel,
Vocos) -> audio, all on the GPU. Differences from the reference:
- `from_features` calls the model without `previous_samples`, which the
  reference's MelGenerator.forward requires (a TypeError there); here it is
  optional and Vocos ignores it.
- `checkpoint=None` runs an untrained (default-initialised) model: there is
  no published Vocos checkpoint. A file or a directory of generator-*.pt
  loads as in promonet_amd.synthesize.
- There is no CPU path: `gpu=None` takes the device of a GPU tensor and
  raises for a CPU one.
- `from_files_to_files_batched` (no reference counterpart) reconstructs
  `batch_size` files per ragged Vocos forward; same files, same bytes as
  `from_files_to_files`.
- Audio at another rate is resampled on the device (pm_resample); the
  reference resamples on the host (mels.py:174-).
"""
from pathlib import Path

import torch

import promonet_amd


###############################################################################
# Mel spectrogram reconstruction
###############################################################################


def from_audio(
    audio,
    sample_rate=promonet_amd.SAMPLE_RATE,
    speaker=0,
    spectral_balance_ratio: float = 1.,
    loudness_ratio: float = 1.,
    checkpoint=None,
    gpu=None
):
    """Perform Mel spectrogram reconstruction: (1, N) audio -> (1, 256 T)"""
    device = _device(gpu, audio)
    audio = resample(audio.to(device), sample_rate)
    spectrogram = promonet_amd.preprocess.spectrogram.from_audio(audio)
    return from_features(
        spectrogram,
        speaker,
        spectral_balance_ratio,
        loudness_ratio,
        checkpoint)


def from_features(
    spectrogram,
    speaker=0,
    spectral_balance_ratio: float = 1.,
    loudness_ratio: float = 1.,
    checkpoint=None
):
    """Perform Mel spectrogram reconstruction: (513, T) -> (1, 256 T)"""
    device = spectrogram.device
    promonet_amd._lib.require_gpu(spectrogram)

    model = _model(checkpoint, device)

    speakers = torch.full((1,), speaker, dtype=torch.long, device=device)
    spectral_balance_ratio = torch.tensor(
        [spectral_balance_ratio], dtype=torch.float, device=device)
    loudness_ratio = torch.tensor(
        [loudness_ratio], dtype=torch.float, device=device)
    with torch.inference_mode():
        return model(
            spectrogram[None],
            speakers,
            spectral_balance_ratio,
            loudness_ratio
        )[0].to(torch.float32)


def from_file(
    audio_file,
    speaker=0,
    spectral_balance_ratio: float = 1.,
    loudness_ratio: float = 1.,
    checkpoint=None,
    gpu=None
):
    """Perform Mel reconstruction from audio file"""
    return from_audio(
        promonet_amd.load.audio(audio_file, gpu=gpu),
        speaker=speaker,
        spectral_balance_ratio=spectral_balance_ratio,
        loudness_ratio=loudness_ratio,
        checkpoint=checkpoint,
        gpu=gpu)


def from_file_to_file(
    audio_file,
    output_file,
    speaker=0,
    spectral_balance_ratio: float = 1.,
    loudness_ratio: float = 1.,
    checkpoint=None,
    gpu=None
):
    """Perform Mel reconstruction from audio file and save"""
    reconstructed = from_file(
        audio_file,
        speaker,
        spectral_balance_ratio,
        loudness_ratio,
        checkpoint,
        gpu)
    promonet_amd.synthesize.core.save_audio(output_file, reconstructed.cpu())


def from_files_to_files(
    audio_files,
    output_files,
    speakers=None,
    spectral_balance_ratio: float = 1.,
    loudness_ratio: float = 1.,
    checkpoint=None,
    gpu=None
):
    """Perform Mel reconstruction from audio files and save"""
    if speakers is None:
        speakers = [0] * len(audio_files)
    for item in zip(audio_files, output_files, speakers):
        from_file_to_file(
            *item,
            spectral_balance_ratio=spectral_balance_ratio,
            loudness_ratio=loudness_ratio,
            checkpoint=checkpoint,
            gpu=gpu)


def from_files_to_files_batched(
    audio_files,
    output_files,
    speakers=None,
    spectral_balance_ratio: float = 1.,
    loudness_ratio: float = 1.,
    checkpoint=None,
    gpu=None,
    batch_size=32
):
    """`from_files_to_files` with `batch_size` files per forward instead of
    the reference's one-file loop (mels.py:146-166); same files, same audio.
    Each utterance's spectrogram is taken on its own (`from_audio` reflect-pads
    its ends), the (513, T_b) spectrograms are zero-padded into one batch and
    run as one ragged forward, and 256 T_b samples are written per file. The
    files of a batch are decoded on the host, grouped by native rate and
    resampled one group per ragged launch, one row per channel (`_load_batch`).
    Runs in this process."""
    count = len(audio_files)
    if count == 0:
        return
    if gpu is None:
        raise RuntimeError(
            'promonet_amd.baseline.mels runs on an AMD GPU only: pass '
            'gpu=<index> (no CPU fallback)')
    if batch_size < 1:
        raise ValueError('batch_size must be positive')
    device = torch.device(f'cuda:{gpu}')
    if speakers is None:
        speakers = [0] * count
    model = _model(checkpoint, device)
    hop = promonet_amd.HOPSIZE
    decoded = [promonet_amd.load.decode(file) for file in audio_files]
    frames = [_resampled_length(rate, data.shape[-1]) // hop
              for rate, data in decoded]
    # (longest first: the engine's workspace is sized once, not per batch)
    order = sorted(range(count), key=lambda index: (-frames[index], index))
    for start in range(0, count, batch_size):
        group = order[start:start + batch_size]
        audio = _load_batch([decoded[index] for index in group], device)
        spectrograms = torch.zeros(
            len(group), promonet_amd.NUM_FFT // 2 + 1, frames[group[0]],
            device=device)
        for row, index in enumerate(group):
            spectrograms[row, :, :frames[index]] = \
                promonet_amd.preprocess.spectrogram.from_audio(audio[row])
        size = (len(group),)
        with torch.inference_mode():
            reconstructed = model(
                spectrograms,
                torch.tensor(
                    [speakers[index] for index in group], dtype=torch.long,
                    device=device),
                torch.full(
                    size, spectral_balance_ratio, dtype=torch.float,
                    device=device),
                torch.full(
                    size, loudness_ratio, dtype=torch.float, device=device),
                lengths=[frames[index] for index in group]
            ).to(torch.float32).cpu()
        for row, index in enumerate(group):
            promonet_amd.synthesize.core.save_audio(
                output_files[index],
                reconstructed[row, :, :frames[index] * hop])


###############################################################################
# Utilities
###############################################################################


def _model(checkpoint, device):
    """The cached MelGenerator (mels.py:54-70)"""
    if (
        not hasattr(from_features, 'model') or
        from_features.checkpoint != checkpoint or
        from_features.device != device
    ):
        model = promonet_amd.model.MelGenerator()
        if checkpoint is not None:
            file = Path(checkpoint)
            if file.is_dir():
                files = sorted(file.glob('generator-*.pt'))
                if not files:
                    raise FileNotFoundError(f'no generator-*.pt in {file}')
                file = files[-1]
            promonet_amd.synthesize.core.load_checkpoint(file, model)
        from_features.model = model.to(device).eval()
        from_features.checkpoint = checkpoint
        from_features.device = device
    return from_features.model



def resample(audio, sample_rate):
    """Resample audio to the ProMoNet sample rate (promonet_amd.load.resample:
    a device tensor stays on the device, mels.py:174-)"""
    if int(sample_rate) == promonet_amd.SAMPLE_RATE:
        return audio
    return promonet_amd.load.resample(
        audio, sample_rate, promonet_amd.SAMPLE_RATE)


def _resampled_length(rate, samples):
    """Samples of `samples` at `rate` once at the ProMoNet sample rate"""
    if int(rate) == promonet_amd.SAMPLE_RATE:
        return samples
    orig, new, _, _ = promonet_amd.load.resample_geometry(
        rate, promonet_amd.SAMPLE_RATE)
    return (new * samples + orig - 1) // orig


def _load_batch(decoded, device):
    """`promonet_amd.load.audio(file, gpu)` of every (rate, (channels,
    samples)) item of promonet_amd.load.decode, bit for bit: the items of one
    native rate are zero-padded into one (rows, longest) upload, one row per
    channel, and resampled in one ragged launch; an item at the ProMoNet rate
    never reaches the resampler."""
    result = [None] * len(decoded)
    rates = {}
    for index, (rate, data) in enumerate(decoded):
        if int(rate) == promonet_amd.SAMPLE_RATE:
            result[index] = data.mean(dim=0, keepdim=True).to(device)
        else:
            rates.setdefault(int(rate), []).append(index)
    for rate, members in rates.items():
        longest = max(decoded[index][1].shape[-1] for index in members)
        rows = sum(decoded[index][1].shape[0] for index in members)
        batch = torch.zeros(rows, longest)
        lengths, row = [], 0
        for index in members:
            data = decoded[index][1]
            batch[row:row + data.shape[0], :data.shape[-1]] = data
            lengths += [data.shape[-1]] * data.shape[0]
            row += data.shape[0]
        resampled, out_lengths = promonet_amd.load.resample(
            batch.to(device), rate, promonet_amd.SAMPLE_RATE, lengths=lengths)
        row = 0
        for index in members:
            channels = decoded[index][1].shape[0]
            result[index] = promonet_amd.load.mono(
                resampled[row:row + channels, :out_lengths[row]])
            row += channels
    return result


def _device(gpu, audio):
    if gpu is not None:
        return torch.device(f'cuda:{gpu}')
    if audio.is_cuda:
        return audio.device
    raise RuntimeError(
        'promonet_amd.baseline.mels runs on an AMD GPU only: pass gpu=<index> '
        '(no CPU fallback)')

