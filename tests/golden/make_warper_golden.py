"""Writes tests/golden/warper_pins.pt: the kept masks of transformers' chained logits warpers (TemperatureLogitsWarper ->
TopKLogitsWarper -> TopPLogitsWarper -> MinPLogitsWarper, min_tokens_to_keep = 1) on 8 rows at V = 1000 -- one row of each
tie-free kind, four bf16-rounded rows -- for every parameter set of tests/warper_cases.py GRID, bit-packed.  Needs
``transformers``; the GPU tests read only the file.

    python tests/golden/make_warper_golden.py"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import warper_cases as W  # noqa: E402

V = 1000


def pin_rows():
    rows = [W.make_rows(kind, 1, V, seed_offset=1) for kind in W.TIE_FREE] + [W.make_rows("bf16", 4, V, seed_offset=1)]
    return torch.cat(rows, 0)


def main():
    import transformers
    x = pin_rows()
    kept = torch.stack([W.pack(W.transformers_kept(x, *prm)) for prm in W.GRID], 0)
    torch.save({"logits": x, "tie_free_rows": len(W.TIE_FREE), "params": [tuple(p) for p in W.GRID], "kept": kept,
                "transformers": transformers.__version__}, os.path.join(HERE, "warper_pins.pt"))
    print(f"{kept.shape[0]} parameter sets x {x.shape[0]} rows, {kept.numel() + x.numel() * 4} bytes of payload")


if __name__ == "__main__":
    main()
