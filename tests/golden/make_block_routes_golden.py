"""Records tests/golden/block_routes.json.  Run ONCE, on an MI355X, in a checkout of 2f9617b (the commit before SynthesisBlock's device forms got one route
decision, modconv.block_route) with tests/block_trace.py of this tree beside it:

    python tests/golden/make_block_routes_golden.py

Every case of block_trace.cases() runs G.synthesis under torch.no_grad() with the replayed uniforms of the small-ray model goldens: one warm-up pass, then two
traced ones.  Stored: the second pass's records (each distinct record once, a case as a list of indices) and the SHA-256 of each output's bytes; an output
whose two digests differ is listed under that case's ``unstable`` instead (none may be image_raw / image_depth of a 'const' / 'none' case)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import block_trace as T  # noqa: E402


def main():
    records, index, cases = [], {}, {}
    for case_id, case in T.cases().items():
        events, (first, second) = T.run_case(case)
        trace = []
        for ev in events:
            key = json.dumps(ev, sort_keys=True)
            if key not in index:
                index[key] = len(records)
                records.append(ev)
            trace.append(index[key])
        unstable = sorted(k for k in T.OUTPUTS if first[k] != second[k])
        assert case['noise_mode'] == 'random' or not {'image_raw', 'image_depth'} & set(unstable), (case_id, unstable)
        cases[case_id] = dict(trace=trace, digests={k: v for k, v in second.items() if k not in unstable}, unstable=unstable)
        print(case_id, len(trace), 'records', 'unstable:', unstable, flush=True)
    with open(T.GOLDEN_FILE, 'w') as f:
        json.dump(dict(records=records, cases=cases), f, separators=(',', ':'), sort_keys=True)
    print('distinct records', len(records), 'bytes', os.path.getsize(T.GOLDEN_FILE))


if __name__ == '__main__':
    main()
