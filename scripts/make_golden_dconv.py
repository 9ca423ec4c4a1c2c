"""Write tests/golden/dconv.pt from the real reference (build host only).

Imports the reference with oracle/reference_import.py, builds its own
`DiscriminatorCMB()` (promonet/model/discriminator.py:146-208) and
`DiscriminatorR((1024, 120, 600))` (:96-127), loads the closed-form parameters
of tests/dconv_oracle.py (`parameters`) into them and runs `band_convs` /
`conv_post` (and `convs` / `conv_post`) in float64 on given tensors, fed to
the layers directly: for CMB the five band slices of the fixed (2, 1, 6, 513)
tensor, for R the fixed (2, 1, 33, 21) tensor (`stack_input`). The gradients
are autograd's, of a fixed linear functional of every map (`coefficients`,
mended at the fragile elements: `stack_backward`), in the inputs and in every
weight_g / weight_v / bias. The script asserts that the float64 restatement
equals all of it to 1e-12 of each tensor's largest value.

Kept: the inputs, the logits, every MAP_STRIDE-th element of each flattened
map, every GRADIENT_STRIDE-th element of each weight_v gradient, the other
gradients whole, where and by what the functional was mended, and both
classes' state_dict keys and shapes. Under 200 KB.

    python scripts/make_golden_dconv.py
"""
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / 'oracle'))
sys.path.insert(0, str(ROOT / 'tests'))

MAP_STRIDE, GRADIENT_STRIDE = 131, 127
RESOLUTION = (1024, 120, 600)


def main():
    import reference_import
    import dconv_oracle as oracle
    if not reference_import.available():
        raise SystemExit('the reference is not on this machine')
    promonet = reference_import.load()
    model = promonet.model.discriminator

    def close(got, want):
        scale = want.abs().max()
        assert (got - want).abs().max() <= 1e-12 * scale, (
            (got - want).abs().max(), scale)

    out = {'map_stride': MAP_STRIDE, 'gradient_stride': GRADIENT_STRIDE,
           'resolution': list(RESOLUTION), 'stacks': {}, 'keys': {},
           'shapes': {}}
    for name in ('cmb', 'r'):
        theirs = model.DiscriminatorCMB() if name == 'cmb' \
            else model.DiscriminatorR(RESOLUTION)
        state = theirs.state_dict()
        out['keys'][name] = list(state)
        out['shapes'][name] = [list(v.shape) for v in state.values()]
        if name == 'cmb':
            out['bands'] = [list(band) for band in theirs.bands]
            assert out['bands'] == [list(e) for e in oracle.CMB_EDGES]
        parameters = oracle.parameters(name)
        assert list(parameters) == list(state)
        theirs = theirs.double()
        theirs.load_state_dict(
            {key: value.double() for key, value in parameters.items()},
            strict=True)
        x = oracle.stack_input(name)
        if name == 'cmb':
            inputs = [x[..., low:high] for low, high in oracle.CMB_EDGES]
        else:
            inputs = [x]

        # the restatement, and the functional mended where it is fragile
        logits, maps, saved = oracle.stack(name, inputs, parameters)
        plain = oracle.coefficients(name, [m.shape for m in maps])
        grad_inputs, gradients, coefficients = oracle.stack_backward(
            saved, parameters, plain, mend=True)
        # (map, flat index, value) of the mended coefficients
        mended = [[], [], []]
        for index, (before, after) in enumerate(zip(plain, coefficients)):
            where = (before != after).flatten().nonzero().flatten()
            mended[0].append(torch.full_like(where, index))
            mended[1].append(where)
            mended[2].append(after.flatten()[where])

        # the reference's own layers on the same tensors
        leaves = [v.double().clone().requires_grad_(True) for v in inputs]
        outputs, last = [], []
        if name == 'cmb':
            for band, layers in zip(leaves, theirs.band_convs):
                for layer in layers:
                    band = layer(band)
                    outputs.append(band)
                last.append(band)
            outputs.append(theirs.conv_post(torch.cat(last, dim=-1)))
        else:
            value = leaves[0]
            for layer in theirs.convs:
                value = torch.nn.functional.leaky_relu(layer(value), 0.2)
                outputs.append(value)
            outputs.append(theirs.conv_post(value))
        total = sum((c.double() * o).sum()
                    for c, o in zip(coefficients, outputs))
        total.backward()
        named = dict(theirs.named_parameters())

        close(logits, outputs[-1].detach())
        for mine, their in zip(maps, outputs):
            close(mine, their.detach())
        for mine, leaf in zip(grad_inputs, leaves):
            close(mine, leaf.grad)
        kept = {}
        for key, mine in gradients.items():
            close(mine, named[key].grad)
            step = GRADIENT_STRIDE if key.endswith('weight_v') else 1
            kept[key] = named[key].grad.flatten()[::step]
        strided = [o.detach().flatten()[::MAP_STRIDE] for o in outputs[:-1]]
        out['stacks'][name] = {
            'x': x.clone(),
            'logits': outputs[-1].detach().clone(),
            # (few tensors: each costs the file more than its bytes)
            'maps': torch.cat(strided),
            'map_counts': [len(v) for v in strided],
            'map_shapes': [list(o.shape) for o in outputs],
            'mended': [torch.cat(column) for column in mended],
            'gradient_x': torch.cat([leaf.grad for leaf in leaves], dim=-1),
            'gradients': torch.cat(list(kept.values())),
            'gradient_counts': [(key, len(v)) for key, v in kept.items()]}
        print(f'{name}: the oracle equals the reference; '
              f'{sum(len(w) for w in mended[1])} coefficients mended')
    path = ROOT / 'tests' / 'golden' / 'dconv.pt'
    torch.save(out, path)
    size = path.stat().st_size
    assert size < 200 * 1024, size
    print(f'{path}: {size} bytes')


if __name__ == '__main__':
    main()
