#!/usr/bin/env python3
"""KITTI-2015 (train) validation of raft_large / raft_small: EPE and F1-all over the valid pixels.

  python scripts/validate_kitti.py /path/to/KITTI [--model raft_large] [--weights w.msgpack]
      [--iters 24] [--max-pairs N]

Multi-GPU (data-parallel, one rank per GPU over RCCL):
  torchrun --nproc-per-node 8 --master-addr 127.0.0.1 scripts/validate_kitti.py /path/to/KITTI
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from jax_raft_amd.cli import validate_kitti_main  # noqa: E402

if __name__ == "__main__":
    sys.exit(validate_kitti_main())
