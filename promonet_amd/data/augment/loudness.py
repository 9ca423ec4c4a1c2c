"""promonet/data/augment/loudness.py: loudness shifts that do not clip."""
import promonet_amd


def _shift(audio, ratio):
    """preprocess.loudness.shift by the ratio in decibels: pm_loudness_shift
    for device audio, the same product on the host otherwise"""
    db = promonet_amd.convert.ratio_to_db(float(ratio))
    if audio.is_cuda:
        return promonet_amd.preprocess.loudness.shift(audio, db)
    return audio * promonet_amd.convert.db_to_ratio(db)


def _shift_without_clipping(audio, ratio):
    """(shifted audio, the ratio that was used): the ratio is drawn again
    while any sample reaches +-1. One reduction and one host read per trial:
    the next draw depends on it, as in the reference's loop."""
    augmented = _shift(audio, ratio)
    while ((augmented <= -1.) | (augmented >= 1.)).any().item():
        ratio = promonet_amd.data.augment.sample(1)[0]
        augmented = _shift(audio, ratio)
    return augmented, ratio


def from_audio(audio, sample_rate, ratio, gpu=None):
    """Perform volume data augmentation on audio (channels, samples); returns
    (audio at SAMPLE_RATE, the ratio used)"""
    if gpu is not None:
        audio = audio.to(f'cuda:{gpu}')
    augmented, ratio = _shift_without_clipping(audio.float(), ratio)
    augmented = promonet_amd.resampy.resample(
        augmented, sample_rate, promonet_amd.SAMPLE_RATE)
    return augmented, ratio


def from_file(audio_file, ratio, gpu=None):
    """Perform volume data augmentation on audio file"""
    rate, audio = promonet_amd.load.decode(audio_file)
    return from_audio(audio, rate, ratio, gpu=gpu)


def _renamed(output_file, ratio, new_ratio):
    """The output file once the ratio in its name was drawn again"""
    if new_ratio == ratio:
        return output_file
    return output_file.parent / output_file.name.replace(
        f'{int(ratio * 100):03d}', f'{int(new_ratio * 100):03d}')


def from_file_to_file(audio_file, output_file, ratio, gpu=None):
    """Perform volume data augmentation on audio file and save; returns the
    ratio used, which the file's name carries"""
    augmented, new_ratio = from_file(audio_file, ratio, gpu=gpu)
    promonet_amd.synthesize.save_audio(
        _renamed(output_file, ratio, new_ratio), augmented)
    return new_ratio


def from_files_to_files(audio_files, output_files, ratios, gpu=None):
    """Perform volume data augmentation on audio files and save; returns the
    ratios used. Every file is shifted (and its ratio drawn again) on its
    own, in order, so the draws are those of the `from_file_to_file` loop;
    the resample to SAMPLE_RATE runs as one ragged batch per native rate."""
    items, used = [], []
    for file, ratio in zip(audio_files, ratios):
        rate, audio = promonet_amd.load.decode(file)
        if gpu is not None:
            audio = audio.to(f'cuda:{gpu}')
        augmented, new_ratio = _shift_without_clipping(audio.float(), ratio)
        items.append((augmented, rate))
        used.append(new_ratio)
    for rate, indices, rows, lengths, owner in (
            promonet_amd.data.augment.batches(items)):
        rows, lengths = promonet_amd.resampy.resample(
            rows, rate, promonet_amd.SAMPLE_RATE, lengths=lengths)
        rows = rows.cpu()
        for index in indices:
            mine = [row for row, item in enumerate(owner) if item == index]
            promonet_amd.synthesize.save_audio(
                _renamed(output_files[index], ratios[index], used[index]),
                rows[mine, :lengths[mine[0]]])
    return used
