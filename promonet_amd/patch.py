"""`promonet_amd.patch(promonet)`: swap the HIP engine into an installed
reference package, the literal drop-in.

After patching, `promonet.synthesize.from_features(..., gpu=N)`,
`promonet.model.Generator()` and `promonet.preprocess.spectrogram.from_audio`
/ `promonet.preprocess.loudness.from_audio` / `limit` / `scale` / `shift` run on
libpromonet_hip.so, and,
where the target has them, `promonet.model.Vocos` / `MelGenerator`,
`promonet.baseline.mels.*` and the `spectrogram` methods of
`promonet.model.discriminator` (DiscriminatorR, DiscriminatorCMB,
SpecDiscriminatorBase; a CPU tensor still takes the target's own method) and
`SpecDiscriminatorBase.forward`, which runs a stack of weight-normed 3x3 convs
of stride 1 and 16 channels under the frequency embedding on the device
(DiscriminatorMagFree at n_fft 64) and leaves every other stack to the
target's own method, and the `forward` of DiscriminatorCMB, DiscriminatorR
and DiscriminatorP, which run their conv stacks on the device where every
layer has one of the reference's forms, and the `forward` of
`promonet.model.hifigan.Block`, which runs its convs on the device in both
directions where autograd is on (model/hifigan_train.py).
"""
import promonet_amd


def patch(promonet):
    """Monkey-patch the reference package object in place and return it."""
    for name in dir(promonet_amd.config):
        if name.isupper() and hasattr(promonet, name) and name not in (
                'ASSETS_DIR', 'AUGMENT_DIR', 'CACHE_DIR', 'ROOT_DIR',
                'COMPUTE_DTYPE'):
            value = getattr(promonet, name)
            if getattr(promonet_amd, name) != value:
                promonet_amd.configure(**{name: value})

    promonet.model.HiFiGAN = promonet_amd.model.HiFiGAN
    promonet.model.FARGAN = promonet_amd.model.FARGAN
    promonet.model.Generator = promonet_amd.model.Generator
    for name in (
        'from_features', 'from_file', 'from_file_to_file',
        'from_files_to_files', 'generate'
    ):
        setattr(promonet.synthesize, name,
                getattr(promonet_amd.synthesize, name))
        if hasattr(promonet.synthesize, 'core'):
            setattr(promonet.synthesize.core, name,
                    getattr(promonet_amd.synthesize, name))
    promonet.preprocess.spectrogram.from_audio = \
        promonet_amd.preprocess.spectrogram.from_audio
    promonet.preprocess.spectrogram.linear_to_mel = \
        promonet_amd.preprocess.spectrogram.linear_to_mel
    promonet.preprocess.loudness.from_audio = \
        promonet_amd.preprocess.loudness.from_audio
    # the editing utilities, where the target has them (every release of the
    # reference does; a stand-in of its layout may not)
    for name in ('limit', 'scale', 'shift'):
        if hasattr(promonet.preprocess.loudness, name):
            setattr(promonet.preprocess.loudness, name,
                    getattr(promonet_amd.preprocess.loudness, name))
    # the mel vocoder, only where the target has it
    for name in ('Vocos', 'MelGenerator'):
        if hasattr(promonet.model, name):
            setattr(promonet.model, name, getattr(promonet_amd.model, name))
    # the spectrograms of the spectral discriminators, where the target has
    # them, and SpecDiscriminatorBase.forward for the stacks whose layers the
    # kernels compute (stride 1, 16 channels: DiscriminatorMagFree at n_fft
    # 64), and the forward of DiscriminatorCMB / R / P for the reference's
    # layer forms; every other conv stack stays the target's own
    discriminator = getattr(promonet.model, 'discriminator', None)
    if discriminator is not None:
        promonet_amd.model.discriminator.patch_module(discriminator)
    # the convs of the generator's MRF Blocks under autograd (training), where
    # the target has the module; its own forward everywhere else
    hifigan = getattr(promonet.model, 'hifigan', None)
    if hifigan is not None:
        promonet_amd.model.hifigan_train.patch_module(hifigan)
    mels = getattr(getattr(promonet, 'baseline', None), 'mels', None)
    if mels is not None:
        for name in (
            'from_audio', 'from_features', 'from_file', 'from_file_to_file',
            'from_files_to_files', 'resample'
        ):
            if hasattr(mels, name):
                setattr(mels, name, getattr(promonet_amd.baseline.mels, name))
    return promonet
