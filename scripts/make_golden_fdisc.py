"""Write tests/golden/fdisc.pt from the real reference (build host only).

Imports the reference with oracle/reference_import.py, builds its own
`DiscriminatorMagFree([64, 16, 64])` (promonet/model/discriminator.py:320-389),
the one resolution whose six layers all have stride 1 and 16 channels
(seeded), rounds the parameters to fp32 and runs `self.layers` in float64
on a given (2, 33, 5) tensor, fed to the layers directly, so the mocked
torchaudio of the spectrogram plays no part. The
gradients are autograd's, of a fixed linear functional of the logits and the
five maps, in the input and in every weight_g / weight_v / bias. The script
asserts that the float64 restatement (tests/fdisc_oracle.py) equals all of it
to 1e-12 relative (of the largest value of the tensor).

Kept: the parameters as fp32, the input (the functional's coefficients are
oracle.coefficients), the logits, every MAP_STRIDE-th element of each flattened map, the gradients
(every GRADIENT_STRIDE-th element of those in weight_v), and for all six sizes
the state_dict's keys and shapes and the reference's plan (at 128 ... 2048
its layers have a frequency stride of 2 and 32 ... 256 channels). Under
200 KB.

    python scripts/make_golden_fdisc.py
"""
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / 'oracle'))
sys.path.insert(0, str(ROOT / 'tests'))

MAP_STRIDE, GRADIENT_STRIDE = 7, 3
RESOLUTION = [64, 16, 64]
SEEDS = (0,)
SIZES = (64, 128, 256, 512, 1024, 2048)
FRAMES = 5


def main():
    import reference_import
    import fdisc_oracle as oracle
    if not reference_import.available():
        raise SystemExit('the reference is not on this machine')
    promonet = reference_import.load()
    model = promonet.model.discriminator

    def close(got, want):
        scale = want.abs().max()
        assert (got - want).abs().max() <= 1e-12 * scale, (
            (got - want).abs().max(), scale)

    out = {'map_stride': MAP_STRIDE, 'gradient_stride': GRADIENT_STRIDE,
           'plans': {}, 'keys': {}, 'shapes': {}, 'stacks': {}}
    for n_fft in SIZES:
        plan = model.create_3x3_conv_plan(
            6, model.configs['stretch'][n_fft][0],
            model.configs['down'][n_fft][0],
            model.configs['stretch'][n_fft][1], model.configs['down'][n_fft][1])
        out['plans'][n_fft] = [[list(entry) for entry in layer]
                               for layer in plan]
        state = model.DiscriminatorMagFree(
            [n_fft, n_fft // 4, n_fft]).state_dict()
        out['keys'][n_fft] = list(state)
        out['shapes'][n_fft] = [list(v.shape) for v in state.values()]
    resolution = RESOLUTION
    for index in SEEDS:
        torch.manual_seed(index)
        theirs = model.DiscriminatorMagFree(resolution)
        with torch.no_grad():
            # (away from the initial g = |v|, so that weight norm shows)
            for name, parameter in theirs.named_parameters():
                if name.endswith('weight_g'):
                    parameter.mul_(.5 + torch.rand_like(parameter))
        state = theirs.state_dict()
        parameters = {name: value.detach().to(torch.float32).clone()
                      for name, value in theirs.named_parameters()
                      if value.requires_grad}
        theirs = theirs.double()
        theirs.load_state_dict(
            {**state, **parameters}, strict=True)
        bins = resolution[0] // 2 + 1
        generator = torch.Generator().manual_seed(100 + index)
        x = 20. * torch.randn(2, bins, FRAMES, generator=generator) - 40.
        coefficients = oracle.coefficients(2, bins, FRAMES)
        leaf = x.double().clone().requires_grad_(True)
        value, outputs = leaf.unsqueeze(1), []
        for layer in theirs.layers:
            value = layer(value)
            outputs.append(value)
        total = sum((c.double() * o).sum()
                    for c, o in zip(coefficients, outputs))
        total.backward()
        named = dict(theirs.named_parameters())

        # the restatement
        listed = [tuple(parameters[f'layers.{i}.1.{key}']
                        for key in ('weight_g', 'weight_v', 'bias'))
                  for i in range(6)]
        dilations = [entry[1][0] for entry in out['plans'][resolution[0]]]
        assert all(entry[0] == [1, 1] and entry[1][1] == 1 and
                   entry[2] == [entry[1][0], 1]
                   for entry in out['plans'][resolution[0]])
        logits, maps, saved = oracle.stack(
            x.double().unsqueeze(1), listed, dilations)
        grad_x, gradients = oracle.stack_backward(saved, listed, coefficients)
        close(logits, outputs[-1].detach())
        for mine, their in zip(maps, outputs[:-1]):
            close(mine, their.detach())
        close(grad_x[:, 0], leaf.grad)
        kept = {}
        for i, triple in enumerate(gradients):
            for key, mine in zip(('weight_g', 'weight_v', 'bias'), triple):
                name = f'layers.{i}.1.{key}'
                close(mine, named[name].grad)
                step = GRADIENT_STRIDE if key == 'weight_v' else 1
                kept[name] = named[name].grad.flatten()[::step].clone()
        out['stacks'][index] = {
            'resolution': list(resolution),
            'dilations': dilations,
            'parameters': parameters,
            'x': x.unsqueeze(1).clone(),
            'logits': outputs[-1].detach().clone(),
            'maps': [o.detach().flatten()[::MAP_STRIDE].clone()
                     for o in outputs[:-1]],
            'gradient_x': leaf.grad.unsqueeze(1).clone(),
            'gradients': kept}
        print(f'{resolution} seed {index}: the oracle equals the '
              'reference')
    path = ROOT / 'tests' / 'golden' / 'fdisc.pt'
    torch.save(out, path)
    size = path.stat().st_size
    assert size < 200 * 1024, size
    print(f'{path}: {size} bytes')


if __name__ == '__main__':
    main()
