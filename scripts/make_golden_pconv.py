"""Write tests/golden/pconv.pt from the real reference (build host only).

Imports the reference with oracle/reference_import.py, builds its own
`DiscriminatorP(p)` (promonet/model/discriminator.py:57-93) for p = 2, 5 and
11, loads the closed-form parameters of tests/pconv_oracle.py (`parameters`)
into them and runs their `forward` in float64 on the fixed (2, 1, 486) audio
(`stack_audio`): 486 is even, so period 2 reflects nothing, period 5 reflects
4 samples and period 11 reflects 9; the heights are 243 / 98 / 45 at the
input and 3 / 2 / 1 at layers 4 and 5. The gradients are autograd's, of a
fixed linear functional of every map (`coefficients`, mended at the fragile
elements: `stack_backward`), in the audio and in every weight_g / weight_v /
bias. The script asserts that the float64 restatement equals all of it to
1e-12 of each tensor's largest value, and that no more than 0.1 % of the
pre-activations of a stack are fragile.

Kept: the audio, the logits, every MAP_STRIDE-th element of each flattened
map, every GRADIENT_STRIDE-th element of each weight_v gradient, the other
gradients whole (the audio's among them), where and by what the functional
was mended, and the state_dict keys and shapes of DiscriminatorP and of the
default configuration's Discriminator. Under 300 KB.

    python scripts/make_golden_pconv.py
"""
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / 'oracle'))
sys.path.insert(0, str(ROOT / 'tests'))

MAP_STRIDE, GRADIENT_STRIDE = 131, 4099


def main():
    import reference_import
    import pconv_oracle as oracle
    if not reference_import.available():
        raise SystemExit('the reference is not on this machine')
    promonet = reference_import.load()
    model = promonet.model.discriminator

    def close(got, want):
        scale = want.abs().max()
        assert (got - want).abs().max() <= 1e-12 * scale, (
            (got - want).abs().max(), scale)

    assert promonet.LRELU_SLOPE == oracle.SLOPE
    out = {'map_stride': MAP_STRIDE, 'gradient_stride': GRADIENT_STRIDE,
           'periods': list(oracle.PERIODS), 'stacks': {}}
    whole = model.Discriminator().state_dict()
    out['discriminator_keys'] = list(whole)
    out['discriminator_shapes'] = [list(v.shape) for v in whole.values()]
    audio = oracle.stack_audio()
    out['audio'] = audio.clone()
    for period in oracle.PERIODS:
        theirs = model.DiscriminatorP(period)
        state = theirs.state_dict()
        out['keys'] = list(state)
        out['shapes'] = [list(v.shape) for v in state.values()]
        parameters = oracle.parameters(period)
        assert list(parameters) == list(state)
        theirs = theirs.double()
        theirs.load_state_dict(
            {key: value.double() for key, value in parameters.items()},
            strict=True)

        # the restatement, and the functional mended where it is fragile
        logits, maps, saved = oracle.stack(period, audio, parameters)
        share = oracle.fragile_share(saved)
        assert share <= 1e-3, share
        plain = oracle.coefficients(period, [m.shape for m in maps])
        grad_audio, gradients, coefficients = oracle.stack_backward(
            saved, parameters, plain, mend=True)
        # (map, flat index, value) of the mended coefficients
        mended = [[], [], []]
        for index, (before, after) in enumerate(zip(plain, coefficients)):
            where = (before != after).flatten().nonzero().flatten()
            mended[0].append(torch.full_like(where, index))
            mended[1].append(where)
            mended[2].append(after.flatten()[where])

        # the reference's own forward on the same audio
        leaf = audio.double().clone().requires_grad_(True)
        flat, outputs = theirs(leaf)
        assert torch.equal(flat, torch.flatten(outputs[-1], 1, -1))
        total = sum((c.double() * o).sum()
                    for c, o in zip(coefficients, outputs))
        total.backward()
        named = dict(theirs.named_parameters())

        close(logits, outputs[-1].detach())
        for mine, their in zip(maps, outputs):
            close(mine, their.detach())
        close(grad_audio, leaf.grad)
        kept = {}
        for key, mine in gradients.items():
            close(mine, named[key].grad)
        for key in state:
            step = GRADIENT_STRIDE if key.endswith('weight_v') else 1
            kept[key] = named[key].grad.flatten()[::step]
        strided = [o.detach().flatten()[::MAP_STRIDE] for o in outputs[:-1]]
        out['stacks'][period] = {
            'logits': outputs[-1].detach().clone(),
            # (few tensors: each costs the file more than its bytes)
            'maps': torch.cat(strided),
            'map_counts': [len(v) for v in strided],
            'map_shapes': [list(o.shape) for o in outputs],
            'mended': [torch.cat(column) for column in mended],
            'gradient_audio': leaf.grad.clone(),
            'gradients': torch.cat(list(kept.values())),
            'gradient_counts': [(key, len(v)) for key, v in kept.items()],
            'fragile_share': share}
        print(f'period {period}: the oracle equals the reference; fragile '
              f'share {share:.1e}, {sum(len(w) for w in mended[1])} '
              'coefficients mended')
    path = ROOT / 'tests' / 'golden' / 'pconv.pt'
    torch.save(out, path)
    size = path.stat().st_size
    assert size < 300 * 1024, size
    print(f'{path}: {size} bytes')


if __name__ == '__main__':
    main()
