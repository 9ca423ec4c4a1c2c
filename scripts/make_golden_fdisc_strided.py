"""Write tests/golden/fdisc_strided.pt from the real reference (build host
only).

Imports the reference with oracle/reference_import.py and, for each n_fft of
128 ... 2048, builds its own `DiscriminatorMagFree([n, n // 4, n])`
(promonet/model/discriminator.py:320-389), loads the hashed parameters of
tests/fdisc_strided_oracle.py (closed forms of the index, stored nowhere) with
strict=True and runs `self.layers` in float64 on the fixed
(2, 1, n / 2 + 1, 4) map of the oracle, fed to the layers directly, so the
mocked torchaudio of the spectrogram plays no part. The gradients are
autograd's, of the oracle's fixed linear functional of the five maps and the
logits, in the input and in every weight_g / weight_v / bias. The script
asserts that the float64 restatement equals all of it to 1e-12 relative (of
the largest value of the tensor).

Kept per n_fft: the input, the logits, every MAP_STRIDE-th element of each
flattened map, every INPUT_STRIDE-th element of the gradient in the input,
every GRADIENT_STRIDE-th element of each weight_v's gradient and all of those
of weight_g and bias, and the three strides. No parameters. Under 250 KB.

    python scripts/make_golden_fdisc_strided.py
"""
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / 'oracle'))
sys.path.insert(0, str(ROOT / 'tests'))

# (primes: every channel and every tap is met)
MAP_STRIDE, GRADIENT_STRIDE, INPUT_STRIDE = 127, 251, 5
SIZES = (128, 256, 512, 1024, 2048)


def main():
    import reference_import
    import fdisc_strided_oracle as oracle
    if not reference_import.available():
        raise SystemExit('the reference is not on this machine')
    promonet = reference_import.load()
    model = promonet.model.discriminator

    def close(got, want):
        scale = want.abs().max()
        assert (got - want).abs().max() <= 1e-12 * scale, (
            (got - want).abs().max(), scale)

    out = {'map_stride': MAP_STRIDE, 'gradient_stride': GRADIENT_STRIDE,
           'input_stride': INPUT_STRIDE, 'stacks': {}}
    for n_fft in SIZES:
        theirs = model.DiscriminatorMagFree([n_fft, n_fft // 4, n_fft])
        parameters = oracle.parameters(n_fft)
        theirs = theirs.double()
        theirs.load_state_dict(
            dict({key: value.double() for key, value in parameters.items()},
                 filterbank=theirs.state_dict()['filterbank']), strict=True)
        strides = [layer[1].stride[0] for layer in theirs.layers]
        assert strides == [entry[0] for entry in oracle.plan(n_fft)]
        assert all(layer[1].stride[1] == 1 and
                   tuple(layer[1].dilation) == (1, 1) and
                   tuple(layer[1].padding) == (1, 1)
                   for layer in theirs.layers)
        x = oracle.stack_input(n_fft)
        leaf = x.double().clone().requires_grad_(True)
        value, outputs = leaf, []
        for layer in theirs.layers:
            value = layer(value)
            outputs.append(value)
        coefficients = oracle.coefficients([o.shape for o in outputs])
        total = sum((c.double() * o).sum()
                    for c, o in zip(coefficients, outputs))
        total.backward()
        named = dict(theirs.named_parameters())

        # the restatement
        listed = oracle.listed(parameters)
        logits, maps, saved = oracle.stack(x.double(), listed, strides)
        grad_x, gradients = oracle.stack_backward(saved, listed, coefficients)
        close(logits, outputs[-1].detach())
        for mine, their in zip(maps, outputs[:-1]):
            assert mine.shape == their.shape
            close(mine, their.detach())
        close(grad_x, leaf.grad)
        kept = {}
        for i, triple in enumerate(gradients):
            for key, mine in zip(('weight_g', 'weight_v', 'bias'), triple):
                name = f'layers.{i}.1.{key}'
                close(mine, named[name].grad)
                step = GRADIENT_STRIDE if key == 'weight_v' else 1
                kept[name] = named[name].grad.flatten()[::step].clone()
        out['stacks'][n_fft] = {
            'x': x.clone(),
            'logits': outputs[-1].detach().clone(),
            'shapes': [list(o.shape) for o in outputs],
            'maps': [o.detach().flatten()[::MAP_STRIDE].clone()
                     for o in outputs[:-1]],
            'gradient_x': leaf.grad.flatten()[::INPUT_STRIDE].clone(),
            'gradients': kept}
        print(f'{n_fft}: the oracle equals the reference')
    path = ROOT / 'tests' / 'golden' / 'fdisc_strided.pt'
    torch.save(out, path)
    size = path.stat().st_size
    assert size < 250 * 1024, size
    print(f'{path}: {size} bytes')


if __name__ == '__main__':
    main()
