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
    audio = resample(audio, sample_rate).to(device)
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
        promonet_amd.load.audio(audio_file),
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
    run as one ragged forward, and 256 T_b samples are written per file. Runs
    in this process."""
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
    audio = [promonet_amd.load.audio(file) for file in audio_files]
    frames = [item.shape[-1] // hop for item in audio]
    # (longest first: the engine's workspace is sized once, not per batch)
    order = sorted(range(count), key=lambda index: (-frames[index], index))
    for start in range(0, count, batch_size):
        group = order[start:start + batch_size]
        spectrograms = torch.zeros(
            len(group), promonet_amd.NUM_FFT // 2 + 1, frames[group[0]],
            device=device)
        for row, index in enumerate(group):
            spectrograms[row, :, :frames[index]] = \
                promonet_amd.preprocess.spectrogram.from_audio(
                    audio[index].to(device))
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
    """Resample audio to the ProMoNet sample rate (promonet_amd.load.resample,
    on the host)"""
    if int(sample_rate) == promonet_amd.SAMPLE_RATE:
        return audio
    device = audio.device
    return promonet_amd.load.resample(
        audio.cpu(), sample_rate, promonet_amd.SAMPLE_RATE).to(device)


def _device(gpu, audio):
    if gpu is not None:
        return torch.device(f'cuda:{gpu}')
    if audio.is_cuda:
        return audio.device
    raise RuntimeError(
        'promonet_amd.baseline.mels runs on an AMD GPU only: pass gpu=<index> '
        '(no CPU fallback)')

