"""The scenario grid of tests/test_producer_calls.py and the writer of its goldens.

A scenario is one stdin line of tests/cpp/pipeline_calls_dump.cpp: `<kind> <field> <fact> <n> <t> <K|N> <senders> <k> <m>`.  Its text is
everything the tool prints for it: the create code, the arena, the buffer table and every call of run (deal, finish) with all arguments.

The goldens record what mpc-protocols_amd/csrc/capi_pipelines.hip enqueued in commit 6a74103, before the producers' form moved into
csrc/producer_route.hpp.  To write them again from that commit, or to compare any other:

    git show 6a74103:mpc-protocols_amd/csrc/capi_pipelines.hip > /tmp/capi_pipelines_then.hip
    make -B -C tests/cpp pipeline_calls_dump PIPELINES=/tmp/capi_pipelines_then.hip
    python -m tests.producer_calls            # writes tests/golden/producer_calls.txt and producer_calls_forms.txt
    make -B -C tests/cpp pipeline_calls_dump  # the tree's file again
"""
import hashlib
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "pipeline_calls_dump")
GOLDEN = os.path.join(ROOT, "tests", "golden", "producer_calls.txt")
FORMS = os.path.join(ROOT, "tests", "golden", "producer_calls_forms.txt")
EB = {"fr": 32, "gl": 8}
LIM = 2 ** 32 - 1
PARTIES = [(1, 0), (2, 0), (3, 1), (4, 1), (5, 1), (5, 2), (7, 2), (10, 3), (13, 4), (16, 5), (16, 1)]


def around(*xs):
    return {x + d for x in xs for d in (-1, 0, 1) if x + d >= 1}


def batch_sizes(field, n, nver, grouped_by):
    """1, 5 and every threshold of the rule at -1, 0, +1, for nver verifiers of n parties"""
    eb, ks = EB[field], {1, 5} | around(2 ** 19, 2 ** 20 - 1)
    if grouped_by:
        ks |= around(4096 // grouped_by)
    if nver:
        ks |= around(-(-2 ** 32 // (n * nver * eb)))  # the smallest K with n nver K eb >= 2^32
    if n >= 2:
        # the largest K at which a deal call still holds two dealers: min(LIM / (n K eb), LIM / (K (deg + 1) eb)) >= 2, and deg + 1 <= n
        # for both degrees, t and 2t
        ks |= around(LIM // (2 * n * eb))
    return sorted(ks)


def facts(nver):
    return (1, 0) if nver == 2 else (1,)  # the rule reads the fact only for two verifiers


def producer(kind, field, fact, n, t, K, senders=0):
    return "%s %s %d %d %d %d %d 0 0" % (kind, field, fact, n, t, K, senders)


def grid():
    out = []
    for field in ("fr", "gl"):
        for n, t in PARTIES:
            for fact in facts(2 * t):
                for K in batch_sizes(field, n, 2 * t, 2 * t):
                    out += [producer("ransha", field, fact, n, t, K, s) for s in sorted({0, 2 * t + 1, n})]
            for fact in facts(n - t - 1):
                out += [producer("randousha", field, fact, n, t, K) for K in batch_sizes(field, n, n - t - 1, n - t - 1)]
        for n, t in ((31, 10), (64, 21)):
            nver, block = 2 * t, -(-2 ** 32 // (n * 2 * t * EB[field]))  # n - t - 1 == 2t verifiers of either kind; the party-major block's 4 GiB
            assert nver == n - t - 1
            for K in (5, block - 1, block):
                out += [producer("ransha", field, 1, n, t, K, s) for s in (0, n)] + [producer("randousha", field, 1, n, t, K)]
        # refused: n <= 2t, K = 0, verify_senders below 2t + 1 and above n
        out += [producer(kind, field, 1, n, t, 5) for kind in ("ransha", "randousha", "preprocessing") for n, t in ((2, 1), (4, 2))]
        out += [producer(kind, field, 1, 4, 1, 0) for kind in ("ransha", "randousha", "preprocessing")]
        out += [producer("ransha", field, 1, 7, 2, 5, s) for s in (4, 8)]
        # preprocessing: N of whole batch elements on both sides of every cut (the producers write into TripleGen's arrays), and not;
        # at the node's size the producers take the together form
        out += [producer("preprocessing", field, 1, n, t, N) for n, t, N in ((4, 1, 6), (4, 1, 3), (7, 2, 15), (7, 2, 5), (16, 5, 66), (16, 5, 11),
                                                                             (16, 5, 22528))]
        # the single-call pipelines, at two sizes
        for n, t in ((4, 1), (16, 5)):
            for size in (2, 4099):
                out.append(producer("triplegen", field, 1, n, t, size * (2 * t + 1)))
                out.append(producer("randbit", field, 1, n, t, size * (t + 1)))
                out += [producer("mul", field, 1, n, t, size, s) for s in (0, n)]
                if field == "fr":
                    for kind in ("fpmul", "truncpr", "fpdivconst"):
                        out += ["%s fr 1 %d %d %d %d 32 16" % (kind, n, t, size, s) for s in (0, n)]
    out += ["fpmul gl 1 4 1 2 0 32 16", "truncpr gl 1 4 1 2 0 32 16", "mul fr 1 4 1 2 2 0 0", "randbit fr 1 4 1 3 0 0 0", "triplegen fr 1 4 1 4 0 0 0"]
    assert len(out) == len(set(out))
    return out


# name -> scenario: the written record of what each form enqueues (tests/golden/producer_calls_forms.txt holds their full text)
FORM_SCENARIOS = {
    "ransha_none_fr": producer("ransha", "fr", 1, 2, 0, 5),
    "ransha_none_gl": producer("ransha", "gl", 1, 2, 0, 5),
    "ransha_grouped_fr": producer("ransha", "fr", 1, 4, 1, 5),
    "ransha_grouped_gl": producer("ransha", "gl", 1, 7, 2, 1024),
    "ransha_together_fr": producer("ransha", "fr", 1, 7, 2, 1025),
    "ransha_together_gl": producer("ransha", "gl", 1, 7, 2, 1025),
    "ransha_per_verifier_all_senders_fr": producer("ransha", "fr", 1, 7, 2, 1025, 7),
    "ransha_per_verifier_two_verifiers_no_list_kernel_gl": producer("ransha", "gl", 0, 4, 1, 2049),
    "ransha_per_verifier_from_2_19_columns_fr": producer("ransha", "fr", 1, 7, 2, 2 ** 19),
    "ransha_together_below_4_gib_fr": producer("ransha", "fr", 1, 64, 21, 49932),
    "ransha_per_verifier_block_of_4_gib_fr": producer("ransha", "fr", 1, 64, 21, 49933, 64),
    "randousha_grouped_sel_fr": producer("randousha", "fr", 1, 4, 1, 5),
    "randousha_grouped_sel_no_verifier_fr": producer("randousha", "fr", 1, 1, 0, 5),
    "randousha_together_sel_fr": producer("randousha", "fr", 1, 7, 2, 1025),
    "randousha_per_verifier_sel_fr": producer("randousha", "fr", 1, 7, 2, 2 ** 19),
    "randousha_per_verifier_sel_two_verifiers_no_list_kernel_fr": producer("randousha", "fr", 0, 4, 1, 2049),
    "randousha_together_c0_gl": producer("randousha", "gl", 1, 4, 1, 5),
    "randousha_per_verifier_c0_gl": producer("randousha", "gl", 1, 7, 2, 2 ** 19),
    "randousha_per_verifier_c0_two_verifiers_no_list_kernel_gl": producer("randousha", "gl", 0, 4, 1, 5),
    "deal_one_call_per_dealer_fr": producer("ransha", "fr", 1, 4, 1, 2 ** 20),
    "deal_fifteen_dealers_then_one_fr": producer("randousha", "fr", 1, 16, 5, 2 ** 19),
    "preprocessing_in_place_fr": producer("preprocessing", "fr", 1, 4, 1, 6),
    "preprocessing_copies_gl": producer("preprocessing", "gl", 1, 4, 1, 3),
    "triplegen_gl": producer("triplegen", "gl", 1, 4, 1, 6),
    "fpmul_fr": "fpmul fr 1 4 1 2 0 32 16",
    "truncpr_fr": "truncpr fr 1 4 1 2 0 32 16",
    "fpdivconst_fr": "fpdivconst fr 1 4 1 2 4 32 16",
    "mul_gl": producer("mul", "gl", 1, 4, 1, 2),
    "randbit_fr": producer("randbit", "fr", 1, 4, 1, 4),
}


def run(scenarios):
    """scenario -> its text, from the tool as it is built now"""
    p = subprocess.run([BIN], input="".join(s + "\n" for s in scenarios), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]  # ASan / UBSan findings abort with a non-zero code
    texts = ["== " + part for part in p.stdout.split("== ")[1:]]
    assert [x.split("\n", 1)[0][3:] for x in texts] == list(scenarios)
    return dict(zip(scenarios, texts))


def summary_line(scenario, text):
    lines = text.splitlines()
    return "%s | %s %s %s" % (scenario, lines[1].split()[1], lines[-1].split()[1], hashlib.sha256(text.encode()).hexdigest())


def main():
    scenarios = grid()
    assert set(FORM_SCENARIOS.values()) <= set(scenarios), sorted(set(FORM_SCENARIOS.values()) - set(scenarios))
    texts = run(scenarios)
    with open(GOLDEN, "w") as f:
        f.write("".join(summary_line(s, texts[s]) + "\n" for s in scenarios))
    with open(FORMS, "w") as f:
        f.write("".join("## %s\n%s" % (name, texts[s]) for name, s in FORM_SCENARIOS.items()))
    print(len(scenarios), "scenarios;", os.path.getsize(GOLDEN) + os.path.getsize(FORMS), "bytes")


if __name__ == "__main__":
    main()
