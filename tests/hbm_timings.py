"""What fj_timings must say after a call that ran on the global HBM table (path == 1), directly or as the fallback of a partitioned
attempt (csrc/fj_plan.hip: gt_read, gt_fallback) - test infrastructure shared by the files that force that form.

The form records E_START, E_BUILD, E_PPART (right behind E_BUILD) and E_JOIN on one stream: build_phase_ms and join_ms are disjoint
pieces of total_ms, so each is at most total_ms - the conversion to float is monotone, which makes this comparison exact.  A fallback
adds the abandoned attempt's total_ms, at least one kernel launch (microseconds) against a rounding error of nanoseconds: there
total_ms lies strictly above the sum of the form's own two phases."""


def check_hbm_form(lt, what=None):
    assert lt["path"] == 1, (what, lt)
    build, join, total = lt["build_phase_ms"], lt["join_ms"], lt["total_ms"]
    assert total > 0.0, (what, lt)
    if lt["fell_back"]:
        assert total > build + join, (what, lt)
    else:
        assert total >= max(build, join), (what, lt)
