"""hipEvent times of one whole Mamba4Rec optimisation step, three ways on the same GPU in one process:

    python tools/mamba4rec_step_time.py           # B = 256 and 1024, L = 50, d = 64, N = 2, V = 3417, p = 0.5, the layer's defaults

  torch   mamba_step = "torch": calculate_loss / backward / torch.optim.Adam, the default path
  eager   mamba_step = "fused", mamba_step_graph = False: bsarec_mamba4rec_train_step called per step
  graph   mamba_step = "fused": the same call replayed from its captured graph

The protocol and the output are those of tools/lrurec_step_time.py, whose ``main`` this runs on Mamba4RecModel."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from lrurec_step_time import main

if __name__ == "__main__":
    main("Mamba4RecModel", "mamba_step", "mamba4rec_step_time")
