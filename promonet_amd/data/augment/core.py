"""promonet/data/augment/core.py: ratios, file names and the cached JSON."""
import json

import torch

import promonet_amd

__all__ = ['datasets', 'from_files_to_files', 'sample', 'save', 'batches']


def datasets(datasets, gpu=0):
    """Perform data augmentation on cached datasets"""
    for dataset in datasets:

        # Remove cached metadata that may become stale
        for stats_file in (promonet_amd.ASSETS_DIR / 'stats').glob('*.pt'):
            stats_file.unlink()

        # Get files
        directory = promonet_amd.CACHE_DIR / dataset
        audio_files = sorted(directory.rglob('*-100.wav'))

        # Augment
        from_files_to_files(audio_files, dataset, gpu=gpu)


def from_files_to_files(audio_files, name, gpu=None):
    """Perform data augmentation on audio files: `-p123.wav` and `-l087.wav`
    beside every file, the ratios in AUGMENT_DIR / f'{name}-pitch.json' and
    f'{name}-loudness.json'. gpu=None evaluates on the host (slow)."""
    torch.manual_seed(promonet_amd.RANDOM_SEED)

    # Pitch
    ratios = sample(len(audio_files))
    output_files = [
        file.parent /
        f'{file.stem.split("-")[0]}-p{int(ratio * 100):03d}.wav'
        for file, ratio in zip(audio_files, ratios)]
    promonet_amd.data.augment.pitch.from_files_to_files(
        audio_files, output_files, ratios, gpu=gpu)
    promonet_amd.AUGMENT_DIR.mkdir(exist_ok=True, parents=True)
    save(promonet_amd.AUGMENT_DIR / f'{name}-pitch.json', audio_files, ratios)

    # Loudness; ratios that cause clipping are drawn again
    ratios = sample(len(audio_files))
    output_files = [
        file.parent /
        f'{file.stem.split("-")[0]}-l{int(ratio * 100):03d}.wav'
        for file, ratio in zip(audio_files, ratios)]
    ratios = promonet_amd.data.augment.loudness.from_files_to_files(
        audio_files, output_files, ratios, gpu=gpu)
    save(
        promonet_amd.AUGMENT_DIR / f'{name}-loudness.json',
        audio_files,
        ratios)


def sample(n):
    """Sample data augmentation ratios: log-uniform between the two bounds"""
    distribution = torch.distributions.uniform.Uniform(
        torch.log2(torch.tensor(promonet_amd.AUGMENTATION_RATIO_MIN)),
        torch.log2(torch.tensor(promonet_amd.AUGMENTATION_RATIO_MAX)))
    ratios = 2 ** distribution.sample([n])

    # Prevent duplicates: no ratio may print as the original's "100"
    ratios[(ratios * 100).to(torch.int) == 100] += 1

    return ratios


def save(json_file, audio_files, ratios):
    """Cache augmentation ratios"""
    ratio_dict = {}
    for audio_file, ratio in zip(audio_files, ratios):
        key = f'{audio_file.parent.name}/{audio_file.stem.split("-")[0]}'
        ratio_dict[key] = f'{int(ratio * 100):03d}'
    with open(json_file, 'w') as file:
        json.dump(ratio_dict, file, indent=4)


def batches(items):
    """What the file loops share in place of the reference's process pool.
    items: [(audio (channels, samples), native rate)]. Yields, per native
    rate, (indices of its items, rows (total channels, longest) zero-padded,
    the length of every row, the item every row belongs to): one ragged
    launch per resampling pass serves the whole group."""
    by_rate = {}
    for index, (audio, rate) in enumerate(items):
        by_rate.setdefault(int(rate), []).append(index)
    for rate, indices in by_rate.items():
        longest = max(items[index][0].shape[-1] for index in indices)
        rows, lengths, owner = [], [], []
        for index in indices:
            audio = items[index][0]
            samples = audio.shape[-1]
            rows.append(torch.nn.functional.pad(
                audio.to(torch.float32), (0, longest - samples)))
            lengths += [samples] * audio.shape[0]
            owner += [index] * audio.shape[0]
        yield rate, indices, torch.cat(rows), lengths, owner
