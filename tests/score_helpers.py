"""Helpers of the edit-statistics GPU tests (tests/test_score_gpu.py) that are no part of the reference (tests/score_ref.py)."""
import torch

import vistaocr_amd as va


def tiny_model(al):
    """A one-layer model with the closed-form weights of the oracle: seeded, small, and its greedy output is not the reference text."""
    from oracle import closed_form as cf
    hp = dict(input_line_height=30, rds_line_height=30, lstm_input_dim=32, num_lstm_layers=1, num_lstm_hidden_units=32,
              p_lstm_dropout=0.0, num_in_channels=1)
    sd_np = cf.closed_form_state(hp, len(al))
    model = va.CnnOcrModel(alphabet=al, verbose=False, **hp)
    sd = model.state_dict()
    for k, v in sd_np.items():
        sd[k] = torch.from_numpy(v)
    model.load_state_dict(sd)
    return model
