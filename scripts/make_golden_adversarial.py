"""Write tests/golden/adversarial.pt from the real reference (build host only).

Imports the reference with oracle/reference_import.py and runs its own
`promonet.loss.feature_matching`, `discriminator` and `generator` with both
values of ADVERSARIAL_HINGE_LOSS and FEATURE_MATCHING_OMIT_FIRST on small
lists: two discriminators of three pairs of feature maps (a dozen tensors of
at most 1 024 elements) and two pairs of logits. The inputs are multiples of
2^-4 (maps) and 2^-2 (logits) in [-2, 2] and every tensor has a power of two
of elements, so every sum, mean and total is exact in fp32: the reference's
fp32 results are the exact values, and the script asserts that the float64
restatement (tests/adversarial_oracle.py) equals them to the bit.

Also records, as plain lists, the feature-map shapes of the reference's
DiscriminatorP (periods 2, 3, 5, 7, 11), DiscriminatorR (its three
resolutions) and DiscriminatorCMB at B = 1 and the default training
CHUNK_SIZE, for scripts/bench_adversarial.py.

    python scripts/make_golden_adversarial.py
"""
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / 'oracle'))
sys.path.insert(0, str(ROOT / 'tests'))

MAP_SHAPES = (((2, 4, 8, 8), (2, 8, 4, 8), (2, 16, 4, 2)),
              ((2, 8, 64), (2, 16, 32), (2, 1, 16)))
LOGIT_SHAPES = ((2, 64), (2, 16))
PERIODS = (2, 3, 5, 7, 11)
RESOLUTIONS = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))


def recorded_shapes(promonet):
    """Feature-map shapes at B = 1, one list per discriminator"""
    model = promonet.model.discriminator
    audio = torch.zeros(1, 1, promonet.CHUNK_SIZE)
    groups = {
        'period': [model.DiscriminatorP(period) for period in PERIODS],
        'resolution': [model.DiscriminatorR(r) for r in RESOLUTIONS],
        'multiband': [model.DiscriminatorCMB()]}
    shapes = {}
    with torch.no_grad():
        for name, discriminators in groups.items():
            shapes[name] = []
            for discriminator in discriminators:
                logits, maps = discriminator(audio)
                assert maps[-1].flatten(1, -1).shape == logits.shape
                shapes[name].append([list(m.shape) for m in maps])
    return shapes


def main():
    import reference_import
    import adversarial_oracle as oracle
    if not reference_import.available():
        raise SystemExit('the reference is not on this machine')
    promonet = reference_import.load()
    assert not promonet.ADVERSARIAL_HINGE_LOSS
    assert not promonet.FEATURE_MATCHING_OMIT_FIRST
    seed = 0
    maps = {'real': [], 'fake': []}
    for shapes in MAP_SHAPES:
        for side in maps:
            maps[side].append([])
            for shape in shapes:
                seed += 1
                maps[side][-1].append(oracle.grid(shape, 2. ** -4, seed))
    # equal elements (sign 0) in every pair
    for reals, fakes in zip(maps['real'], maps['fake']):
        for real, fake in zip(reals, fakes):
            fake.flatten()[::5] = real.flatten()[::5]
    logits = {'real': [], 'fake': []}
    for shape in LOGIT_SHAPES:
        for side in logits:
            seed += 1
            logits[side].append(oracle.grid(shape, 2. ** -2, seed))
            # the two boundaries of the hinge
            logits[side][-1].flatten()[:2] = torch.tensor([1., -1.])
    out = {'maps': maps, 'logits': logits, 'results': {}}

    def exact(got, want):
        assert want.dtype == torch.float32 and got.dtype == torch.float64
        assert torch.equal(got, want.double()), (got, want)

    for hinge in (False, True):
        for omit_first in (False, True):
            promonet.ADVERSARIAL_HINGE_LOSS = hinge
            promonet.FEATURE_MATCHING_OMIT_FIRST = omit_first
            matching = promonet.loss.feature_matching(
                maps['real'], maps['fake'])
            total, real_losses, fake_losses = promonet.loss.discriminator(
                logits['real'], logits['fake'])
            generator_total, losses = promonet.loss.generator(logits['fake'])
            exact(oracle.feature_matching(
                maps['real'], maps['fake'], omit_first), matching)
            mine = oracle.discriminator(logits['real'], logits['fake'], hinge)
            exact(mine[0], total)
            exact(torch.stack(mine[1]), torch.stack(real_losses))
            exact(torch.stack(mine[2]), torch.stack(fake_losses))
            mine = oracle.generator(logits['fake'], hinge)
            exact(mine[0], generator_total)
            exact(torch.stack(mine[1]), torch.stack(losses))
            out['results'][f'hinge{int(hinge)}/omit{int(omit_first)}'] = {
                'feature_matching': matching,
                'discriminator': total,
                'discriminator_real': torch.stack(real_losses),
                'discriminator_fake': torch.stack(fake_losses),
                'generator': generator_total,
                'generator_losses': torch.stack(losses)}
    promonet.ADVERSARIAL_HINGE_LOSS = False
    promonet.FEATURE_MATCHING_OMIT_FIRST = False
    out['batch_size'] = int(promonet.BATCH_SIZE)
    out['chunk_size'] = int(promonet.CHUNK_SIZE)
    out['shapes'] = recorded_shapes(promonet)
    path = ROOT / 'tests' / 'golden' / 'adversarial.pt'
    torch.save(out, path)
    size = path.stat().st_size
    assert size < 200 * 1024, size
    count = {name: sum(len(s) for s in lists)
             for name, lists in out['shapes'].items()}
    print(f'{path}: {size} bytes; maps recorded per group: {count}')


if __name__ == '__main__':
    main()
