"""What the gradient-accumulation tests share (tests/test_grad_accumulation_gpu.py, the 1-rank window test of
tests/test_dp_nccl_gpu.py): the three micro-batches of a window and the passes that take their gradients one at a time."""
import torch

N = 3
# caption lengths per micro-batch (row 0, row 1): with a 2- or 4-position image prefix the truncated sequence (engine.truncate:
# longest caption + prefix + 2, rounded up to 64) is 64, 128 and 64 positions
LENS = ((9, 11), (70, 41), (23, 30))
SEQ_OF_LENS = (64, 128, 64)


def micro_batches(seed, eos, S, P, d, res=64):
    g = torch.Generator().manual_seed(seed)
    out = []
    for n0, n1 in LENS:
        images = torch.randn(2, 3, res, res, generator=g).to(torch.bfloat16).float()
        caps = torch.full((2, S), eos, dtype=torch.int64)
        caps[0, :n0] = torch.randint(0, 1000, (n0,), generator=g)
        caps[1, :n1] = torch.randint(0, 1000, (n1,), generator=g)
        mask = (torch.rand(2, P, d, generator=g) < 0.9).float() / 0.9
        out.append((images, caps, mask))
    return out


def zero_window(eng):
    for grp in eng.groups:
        grp.grad.zero_()
    eng.micro_steps = 0


def flat_grads(eng):
    return [grp.grad.clone() for grp in eng.groups]


def forward_backward(eng, batches, i):
    images, caps, mask = batches[i]
    out = eng(images.to(eng.device), caps, dropout_mask=mask.to(eng.device))
    assert eng._tape["S"] == SEQ_OF_LENS[i], "the micro-batches no longer differ in their truncated length"
    eng.backward(out.loss)


def take_parts(eng, batches):
    parts = []
    for i in range(N):
        zero_window(eng)
        forward_backward(eng, batches, i)
        parts.append(flat_grads(eng))
    return parts
