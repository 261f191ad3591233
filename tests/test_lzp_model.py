"""tests/lzp_model.py -- LZP restated in plain Python from its description -- against the reference's results recorded in
tests/golden/lzp.json, and the paths the fixture takes: every case the kernels can get wrong is really in it."""
import collections
import hashlib
import json
import os

import lzp_cases
import lzp_model

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lzp.json")))


def md5(b):
    return hashlib.md5(b).hexdigest()


def test_model_reproduces_every_record_and_the_fixture_takes_every_path():
    fwd_paths, inv_paths = collections.Counter(), collections.Counter()
    outputs = {}
    for rec in GOLDEN["stage"]:
        d = lzp_cases.make(rec["recipe"])
        assert md5(d) == rec["input_md5"], rec["recipe"]
        ok, out, paths = lzp_model.forward(d, rec["cap"])
        fwd_paths.update(paths.keys())
        assert int(ok and len(d) > 0) == rec["ok"], rec["recipe"]          # (an empty block: the reference's sequence reports "nothing applied")
        if rec["ok"]:
            assert len(out) == rec["fwd_len"] and md5(out) == rec["fwd_md5"], rec["recipe"]
            if "fwd_hex" in rec:
                assert out.hex() == rec["fwd_hex"]
            outputs[json.dumps(rec["recipe"])] = out
            iok, back, paths = lzp_model.inverse(out, len(d))
            inv_paths.update(paths.keys())
            assert iok and back == d, rec["recipe"]
    d = lzp_cases.make(lzp_cases.SHORT_CAP)
    assert not lzp_model.forward(d, lzp_cases.max_encoded(len(d)) - 1)[0] and lzp_model.forward(d, lzp_cases.max_encoded(len(d)))[0]
    n_ok = 0
    for rec in GOLDEN["inverse"] + GOLDEN["cut"]:
        d = outputs[json.dumps(rec["recipe"])][:rec["cut"]] if "cut" in rec else lzp_cases.make(rec["recipe"])
        assert md5(d) == rec["input_md5"], rec["recipe"]
        ok, out, paths = lzp_model.inverse(d, rec["cap"])
        inv_paths.update(paths.keys())
        assert int(ok and len(d) > 0) == rec["ok"], (rec["recipe"], rec["cap"], rec.get("where"))
        if rec["ok"]:
            n_ok += 1
            assert md5(out) == rec["inv_md5"], (rec["recipe"], rec["cap"])
    assert 3 * n_ok >= len(GOLDEN["inverse"]) + len(GOLDEN["cut"])
    want_fwd = ["refuse_early", "match_len_64", "len_remainder_253", "len_remainder_0", "fe_run_0", "fe_run_1", "fe_run_2", "fe_run_3+",
                "match_to_block_end", "match_whole_word_stop", "tail_bucket_predicts_right",
                "match_overlap_period_1", "match_overlap_period_3", "match_overlap_period_5",
                "fc_no_escape", "fc_escape", "fc_escape_tail", "fc_no_escape_tail", "match_back_to_back",
                "match_1_after_match_mixed_only", "match_2_after_match_mixed_only", "match_3_after_match_mixed_only",
                "match_bucket_stored_1_after_start_mixed_only", "match_bucket_stored_2_after_start_mixed_only",
                "match_bucket_stored_3_after_start_mixed_only",
                "same_batch_bucket", "fc_escape_same_batch", "precheck_passed_match_short",
                "refuse_literal", "refuse_escape", "refuse_fe_run"]
    assert [p for p in want_fwd if p not in fwd_paths] == []
    want_inv = ["refuse_early", "literal", "fc_empty_bucket", "fc_escaped", "match", "match_fe_run", "match_overlap",
                "refuse_end_after_flag", "refuse_end_in_fe_run", "refuse_match_past_end", "refuse_literal"]
    assert [p for p in want_inv if p not in inv_paths] == []
