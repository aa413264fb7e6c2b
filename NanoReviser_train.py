#!/usr/bin/env python3
"""NanoReviser_train.py - the counterpart of the reference's script of this name, served by the MI355X engine: fits the
per-window tail of both models on the device from per-base labels (see nanoreviser_amd/train_cli.py for what is kept and
what is changed)."""
import sys

from nanoreviser_amd.train_cli import main

if __name__ == "__main__":
    sys.exit(main())
