"""Host side of Force_APTAI's `max_phn_seq_len` / `transcript` options: the positional table, the label-to-slot conversion and the
training script's flags.  No GPU."""
import pytest
import torch


def test_positional_table_rows_do_not_depend_on_the_row_count():
    from aptai_amd.modules import PositionalEncoding
    short, long = PositionalEncoding(128, max_len=60).pe, PositionalEncoding(128, max_len=200).pe
    assert tuple(long.shape) == (200, 1, 128)
    assert torch.equal(long[:60], short)
    assert torch.equal(PositionalEncoding(128, max_len=255).pe[:200], long)


def test_labels_to_slots_pads_cuts_and_counts():
    from aptai_amd.force_aptai import labels_to_slots
    lab = torch.tensor([[5, 7, 9, -100, -100, -100], [3, 3, 4, 8, 2, 6]], dtype=torch.int32)
    ids, n = labels_to_slots(lab, 8)                                   # padded to the cap
    assert ids.dtype == torch.int32 and n.dtype == torch.int32 and ids.is_contiguous()
    assert ids.tolist() == [[5, 7, 9, 0, 0, 0, 0, 0], [3, 3, 4, 8, 2, 6, 0, 0]]
    assert n.tolist() == [3, 6]
    ids, n = labels_to_slots(lab, 6)                                   # exactly the cap: row 1 has `cap` labels, one too many
    assert ids.tolist() == [[5, 7, 9, 0, 0, 0], [3, 3, 4, 8, 2, 6]] and n.tolist() == [3, 6]
    ids, n = labels_to_slots(lab.long(), 4)                            # cut to the cap; the counts are those BEFORE the cut
    assert ids.dtype == torch.int32 and ids.tolist() == [[5, 7, 9, 0], [3, 3, 4, 8]]
    assert n.tolist() == [3, 6]
    ids, n = labels_to_slots(torch.full((2, 3), -100, dtype=torch.int32), 5)   # nothing labelled
    assert ids.tolist() == [[0] * 5] * 2 and n.tolist() == [0, 0]


def test_train_script_flags():
    from aptai_amd import train_force_aptai as tf
    a = tf.parse_args(["--pr_model_path", "x"])
    assert a.max_phn_seq_len == 60 and a.transcript == "decoded"
    a = tf.parse_args(["--pr_model_path", "x", "--max_phn_seq_len", "200", "--transcript", "labels", "--max_grad_norm", "1.5"])
    assert a.max_phn_seq_len == 200 and a.transcript == "labels" and a.max_grad_norm == 1.5
    with pytest.raises(SystemExit):
        tf.parse_args(["--pr_model_path", "x", "--transcript", "spoken"])
    cfg = tf.default_cfg()
    assert cfg.max_phn_seq_len == 60 and cfg.transcript == "decoded"
    assert tf.default_cfg(max_phn_seq_len=255).max_phn_seq_len == 255
