# -*- coding: utf-8 -*-
"""Where in each file its score comes from: run_predict.py's command line (the same flags and errors, through its build_args),
but instead of one row per file it writes one row per file and segment (one every 40 ms in the shipped checkpoints) -- the segment's share of the score and what the
segment says on its own (nisqaModel.profile) -- to NISQA_profile.csv in --output_dir, and prints the table.
  python run_profile.py --mode predict_file --pretrained_model weights/nisqa.tar --deg /path/to/file.wav --output_dir /path/out
One process on one GPU; this is a diagnostic loop, not the throughput path (that is run_predict.py)."""
from nisqa_amd.NISQA_model import frame_to_string, nisqaModel
from run_predict import build_args

if __name__ == "__main__":
    nisqa = nisqaModel(build_args())
    print(frame_to_string(nisqa.profile()))
