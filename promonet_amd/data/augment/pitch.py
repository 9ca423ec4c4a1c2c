"""promonet/data/augment/pitch.py: pitch-shifting by resampling."""
import promonet_amd


def _place(audio, gpu):
    return audio if gpu is None else audio.to(f'cuda:{gpu}')


def from_audio(audio, sample_rate, ratio, gpu=None):
    """Perform pitch-shifting data augmentation on audio (channels, samples):
    two resamples, int(ratio * sample_rate) -> sample_rate -> SAMPLE_RATE. A
    device tensor, or gpu, runs them on the device."""
    resample = promonet_amd.resampy.resample
    augmented = resample(
        _place(audio, gpu), int(ratio * sample_rate), sample_rate)
    return resample(augmented, sample_rate, promonet_amd.SAMPLE_RATE)


def from_file(audio_file, ratio, gpu=None):
    """Perform pitch-shifting data augmentation on audio file"""
    rate, audio = promonet_amd.load.decode(audio_file)
    return from_audio(audio, rate, ratio, gpu=gpu)


def from_file_to_file(audio_file, output_file, ratio, gpu=None):
    """Perform pitch-shifting data augmentation on audio file and save"""
    promonet_amd.synthesize.save_audio(
        output_file, from_file(audio_file, ratio, gpu=gpu))


def from_files_to_files(audio_files, output_files, ratios, gpu=None):
    """Perform pitch-shifting data augmentation on audio files and save.
    Files are decoded on the host and grouped by native rate; a group is one
    ragged batch per resampling pass with one ratio per row. The files written
    are byte for byte those of the `from_file_to_file` loop."""
    resample = promonet_amd.resampy.resample
    items = [promonet_amd.load.decode(file)[::-1] for file in audio_files]
    for rate, indices, rows, lengths, owner in (
            promonet_amd.data.augment.batches(items)):
        rates = [int(ratios[index] * rate) for index in owner]
        rows, lengths = resample(
            _place(rows, gpu), rates, rate, lengths=lengths)
        rows, lengths = resample(
            rows, rate, promonet_amd.SAMPLE_RATE, lengths=lengths)
        rows = rows.cpu()
        for index in indices:
            mine = [row for row, item in enumerate(owner) if item == index]
            promonet_amd.synthesize.save_audio(
                output_files[index], rows[mine, :lengths[mine[0]]])
