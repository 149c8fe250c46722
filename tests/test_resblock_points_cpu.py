"""CPU: why tests/test_hip_resblock.py holds the fp16-autocast decoder level to a float64 reference whose rounding point lies behind the skip add.
Both references are the same torch level in float64 with fp16 points at every conv; they differ in ONE placement - torch rounds conv2's output and adds
the skip in a second step, the fused block rounds x + conv2 once.  No kernel and no library is involved, so the distance between the two is a property
of the placements alone: a handful of block outputs within an fp16 ulp of zero change sign, the next block's ReLU mask flips there, and gradients move
by more than the 1e-2 band the level test uses."""
import copy

import torch

from tests.test_hip_resblock import BAND, decoder_level, step, torch_points, with_fused_points


def test_the_two_placements_of_one_rounding_point_are_further_apart_than_the_band():
    level = decoder_level()                                              # seed 5, as the GPU test builds it
    x, gy = torch.randn(2, 64, 17, 18), torch.randn(2, 32, 34, 36)
    fused, torchs = step(level, x, gy, with_fused_points), step(level, x, gy, torch_points)
    err = {n: float((fused[n] - torchs[n]).abs().max() / torchs[n].abs().max()) for n in torchs}
    print("fused points against torch's points:", " ".join(f"{n}={e:.3e}" for n, e in err.items()))
    assert err["y"] < 1e-3                                               # the values agree to an fp16 rounding ...
    assert err["x"] > BAND[True] and max(err.values()) > 2 * BAND[True]          # ... the gradients do not: 2.4e-2 for the input, 4.3e-2 for a weight
    ref = torch_points(copy.deepcopy(level).double())                    # the cause: outputs of the first block whose sign the placement decides
    with torch.no_grad():
        t = ref[0](x.double())
        c1, c2 = ref[1].layers[2], ref[1].layers[5]
        conv2 = c2._conv_forward(torch.relu(c1(torch.relu(t))).half().double(), c2.weight.half().double(), c2.bias.half().double())
        flipped = int(((t + conv2.half().double() > 0) != ((t + conv2).half() > 0)).sum())
    print("block outputs whose sign the placement decides:", flipped, "of", t.numel())
    assert 0 < flipped < 100
