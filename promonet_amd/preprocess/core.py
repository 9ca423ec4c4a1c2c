"""Audio -> (loudness, pitch, periodicity, ppg, harmonics) orchestration.

API of `promonet.preprocess` (promonet/preprocess/core.py). Loudness and the
harmonic contours run on the HIP kernels. Pitch / periodicity (`penn`) and
PPGs (`ppgs`) are third-party neural networks outside the hot-path scope: they
are imported lazily and used as the reference uses them when installed.
'text' and 'speaker' (whisper, WavLM) are evaluation-only in the reference and
raise.
"""
from pathlib import Path

import torch

import promonet_amd


# what `features` may name, in the order the results come back
FEATURES = ('loudness', 'pitch', 'periodicity', 'ppg', 'harmonics')


def from_audio(
    audio,
    sample_rate=None,
    gpu=None,
    features=None,
    loudness_bands=None,
    max_harmonics=None
):
    """Preprocess audio (preprocess/core.py:17-126). Audio at another
    `sample_rate` is resampled to SAMPLE_RATE on the device first
    (promonet_amd.load.resample) and every feature is taken from the
    resampled audio, a device tensor (at SAMPLE_RATE penn and ppgs get the
    caller's tensor as before). The reference hands `sample_rate` to penn and ppgs,
    which resample for themselves, but feeds the audio at its ORIGINAL rate
    to its loudness (core.py:55-61), whose frames then do not line up with
    the other features: a quirk of the reference that is not mirrored here."""
    sample_rate = sample_rate or promonet_amd.SAMPLE_RATE
    features = list(features or promonet_amd.INPUT_FEATURES)
    if loudness_bands is None:
        loudness_bands = promonet_amd.LOUDNESS_BANDS
    if gpu is None:
        raise RuntimeError(
            'promonet_amd preprocessing runs on an AMD GPU: pass gpu=<index>')
    device = torch.device(f'cuda:{gpu}')
    if sample_rate != promonet_amd.SAMPLE_RATE:
        audio = promonet_amd.load.resample(
            audio.to(device), sample_rate, promonet_amd.SAMPLE_RATE)
        sample_rate = promonet_amd.SAMPLE_RATE
    unsupported = set(features) - set(FEATURES)
    if unsupported:
        raise ValueError(
            f'features {sorted(unsupported)} are evaluation-only in the '
            'reference and out of scope here')
    result = []
    if 'loudness' in features:
        result.append(promonet_amd.preprocess.loudness.from_audio(
            audio.to(device), loudness_bands))
    if 'pitch' in features or 'periodicity' in features:
        try:
            import penn
        except ImportError as error:
            raise ImportError(
                'pitch / periodicity extraction needs the third-party `penn` '
                'package (out of scope of promonet_amd)') from error
        pitch, periodicity = penn.from_audio(
            audio, sample_rate=sample_rate,
            hopsize=promonet_amd.convert.samples_to_seconds(
                promonet_amd.HOPSIZE),
            fmin=promonet_amd.FMIN, fmax=promonet_amd.FMAX, batch_size=2048,
            center='half-hop', decoder='viterbi', gpu=gpu)
        if 'pitch' in features:
            result.append(pitch)
        if 'periodicity' in features:
            result.append(periodicity)
    if 'ppg' in features:
        try:
            import ppgs
        except ImportError as error:
            raise ImportError(
                'PPG extraction needs the third-party `ppgs` package (out of '
                'scope of promonet_amd)') from error
        ppg = ppgs.from_audio(audio, sample_rate, gpu=gpu)
        frames = promonet_amd.convert.samples_to_frames(audio.shape[-1])
        if ppg.shape[-1] != frames:
            grid = ppgs.edit.grid.of_length(ppg, frames)
            ppg = ppgs.edit.grid.sample(ppg, grid, 'linear')
        ppg = torch.softmax(torch.log(ppg + 1e-8), -2)
        result.append(ppg)
    if 'harmonics' in features:
        # no pitch prior, as in core.py:111-116
        result.append(promonet_amd.preprocess.harmonics.from_audio(
            audio.to(device), sample_rate, max_harmonics=max_harmonics))
    return tuple(result) if len(result) != 1 else result[0]


def from_file(file, gpu=None, features=None, loudness_bands=None,
              max_harmonics=None):
    """preprocess/core.py:129-166; the file is resampled on the device
    (load.audio(file, gpu)), so every feature gets a device tensor"""
    return from_audio(
        promonet_amd.load.audio(file, gpu=gpu), gpu=gpu, features=features,
        loudness_bands=loudness_bands, max_harmonics=max_harmonics)


def from_file_to_file(
    file,
    output_prefix=None,
    gpu=None,
    features=None,
    loudness_bands=None,
    max_harmonics=None
):
    """Preprocess and save `{prefix}-loudness.pt`, `{prefix}[-viterbi]-pitch.pt`,
    `...-periodicity.pt`, `{prefix}-ppg.pt`, `{prefix}-harmonics.pt`
    (preprocess/core.py:169-224)."""
    file = Path(file)
    features = list(features or promonet_amd.INPUT_FEATURES)
    if output_prefix is None:
        output_prefix = file.parent / file.stem
    outputs = from_file(file, gpu, features, loudness_bands, max_harmonics)
    if not isinstance(outputs, tuple):
        outputs = (outputs,)
    viterbi = '-viterbi' if promonet_amd.VITERBI_DECODE_PITCH else ''
    names = {
        'loudness': '-loudness.pt',
        'pitch': f'{viterbi}-pitch.pt',
        'periodicity': f'{viterbi}-periodicity.pt',
        'ppg': '-ppg.pt',
        'harmonics': '-harmonics.pt'}
    ordered = [f for f in FEATURES if f in features]
    for feature, output in zip(ordered, outputs):
        torch.save(output.cpu(), f'{output_prefix}{names[feature]}')


def from_files_to_files(
    files,
    output_prefixes=None,
    gpu=None,
    features=None,
    loudness_bands=None,
    max_harmonics=None
):
    """preprocess/core.py:227-319. The harmonics come last and, as in
    core.py:303-312, take the pitch file written just before as their prior
    when 'pitch' is among the features, and also save their STFT features as
    `{prefix}-harmonicfeatures.pt`."""
    features = list(features or promonet_amd.INPUT_FEATURES)
    if output_prefixes is None:
        output_prefixes = [None] * len(files)
    others = [feature for feature in features if feature != 'harmonics']
    viterbi = '-viterbi' if promonet_amd.VITERBI_DECODE_PITCH else ''
    for file, prefix in zip(files, output_prefixes):
        file = Path(file)
        if prefix is None:
            prefix = file.parent / file.stem
        if others:
            from_file_to_file(file, prefix, gpu, others, loudness_bands)
        if 'harmonics' in features:
            promonet_amd.preprocess.harmonics.from_file_to_file(
                file,
                f'{prefix}-harmonics.pt',
                pitch_file=(
                    f'{prefix}{viterbi}-pitch.pt' if 'pitch' in features
                    else None),
                output_feature_file=f'{prefix}-harmonicfeatures.pt',
                max_harmonics=max_harmonics,
                gpu=gpu)
