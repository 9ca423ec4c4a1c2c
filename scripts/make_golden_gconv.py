"""Write tests/golden/gconv.pt from the real reference (build host only).

Imports the reference with oracle/reference_import.py, builds its own
`promonet.model.hifigan.Block(32, k)` (promonet/model/hifigan.py:157-218) for
k = 3, 7 and 11, loads the closed-form parameters of tests/gconv_oracle.py
(`parameters`) into them and runs their `forward` in float64 on the seeded
(2, 32, 48) inputs of the oracle's module cases (`module_inputs`), with
autograd under the seeded upstream gradient. The script asserts that the
float64 composition of the oracle equals all of it to 1e-12 of each tensor's
largest value.

Kept: the input and the upstream gradient (fp32), the output and the gradient
in the input whole, every GRADIENT_STRIDE-th element of each weight_v
gradient, the other gradients whole, and the state_dict keys and shapes of the
reference's Block, ResidualBlock and HiFiGAN. Data only, under 400 KB.

    python scripts/make_golden_gconv.py
"""
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / 'oracle'))
sys.path.insert(0, str(ROOT / 'tests'))

GRADIENT_STRIDE = 7


def main():
    import reference_import
    import gconv_oracle as oracle
    if not reference_import.available():
        raise SystemExit('the reference is not on this machine')
    promonet = reference_import.load()
    model = promonet.model.hifigan

    def close(got, want):
        scale = want.abs().max()
        assert (got - want).abs().max() <= 1e-12 * scale, (
            (got - want).abs().max(), scale)

    def keys_and_shapes(module):
        state = module.state_dict()
        return list(state), [list(value.shape) for value in state.values()]

    assert promonet.LRELU_SLOPE == oracle.SLOPE
    assert tuple(zip(promonet.HIFIGAN_RESBLOCK_KERNEL_SIZES, map(
        tuple, promonet.HIFIGAN_RESBLOCK_DILATION_SIZES))) == oracle.BLOCKS
    out = {'gradient_stride': GRADIENT_STRIDE, 'blocks': {}}
    out['residual_keys'], out['residual_shapes'] = keys_and_shapes(
        model.ResidualBlock(oracle.MODULE_CHANNELS))
    out['hifigan_keys'], out['hifigan_shapes'] = keys_and_shapes(
        model.HiFiGAN(113, 258))
    for kernel, dilations in oracle.BLOCKS:
        name = f'block-{kernel}'
        theirs = model.Block(oracle.MODULE_CHANNELS, kernel, dilations)
        keys, shapes = keys_and_shapes(theirs)
        want = oracle.module_truth(name)
        assert list(want['parameters']) == keys
        theirs = theirs.double()
        theirs.load_state_dict(
            {key: value.double() for key, value in want['parameters'].items()},
            strict=True)
        leaf = want['x'].double().requires_grad_(True)
        y = theirs(leaf)
        y.backward(want['upstream'].double())
        named = dict(theirs.named_parameters())
        close(want['forward'], y.detach())
        close(want['gx'], leaf.grad)
        kept = {}
        for key in keys:
            close(want['gradients'][key], named[key].grad)
            step = GRADIENT_STRIDE if key.endswith('weight_v') else 1
            kept[key] = named[key].grad.flatten()[::step]
        out['blocks'][kernel] = {
            'keys': keys, 'shapes': shapes, 'x': want['x'].clone(),
            'upstream': want['upstream'].clone(),
            'forward': y.detach().clone(), 'gx': leaf.grad.clone(),
            # (few tensors: each costs the file more than its bytes)
            'gradients': torch.cat(list(kept.values())),
            'gradient_counts': [(key, len(v)) for key, v in kept.items()]}
        print(f'{name}: the oracle equals the reference')
    path = ROOT / 'tests' / 'golden' / 'gconv.pt'
    torch.save(out, path)
    size = path.stat().st_size
    assert size < 400 * 1024, size
    print(f'{path}: {size} bytes')


if __name__ == '__main__':
    main()
