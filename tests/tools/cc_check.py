"""Plain, sequential Python restatement of the reference's `clust --cluster-mode 1` (connected component): what plasship_clust_connected_* have
to compute wherever they answer, and what the reference does where they refuse.  It stands where the CPU oracle stands for the other modules
and is itself pinned byte for byte to the reference's DBs in tests/golden/cc.tar.gz (tests/test_cc_host.py).  The loops run in the reference's
order, one element after the other, symmetrisation and depth cut included: the order-free form the GPU uses (components, each under its first
member in rank order) is `order_free` below, argued in plass_amd/csrc/clust_cc.hip and checked against this restatement, not assumed by it.

Restated (lib/mmseqs/src): clustering/Clustering.cpp:18-19 (the sequence DB is opened SORT_BY_LENGTH: an id is a position in length order),
clustering/ClusteringAlgorithms.cpp:38-146 (execute(3)), 148-180 (initClustersizes), 334-401 (readInClusterData),
clustering/AlignmentSymmetry.cpp:20-121 (readInData), 123-165 (findMissingLinks), 167-215 (addMissingLinks), 218-223 (sortElements)."""
import bisect
import os
from collections import deque

from clust_check import UINT_MAX, cluster_entries, first_column, read_db, read_index  # noqa: F401


def length_order(seq_index):
    """SORT_BY_LENGTH: (keys in id order, id of every key); id 0 is the longest sequence, ties by key ascending"""
    seq = sorted(seq_index)
    order = sorted(range(len(seq)), key=lambda i: (-seq[i][1], i))
    local_key = [seq[i][0] for i in order]
    return local_key, {k: j for j, k in enumerate(local_key)}


def read_lists(seq_index, result):
    """the lists as AlignmentSymmetry::readInData fills them, per id, in line order: an entry without lines is the list of the sequence itself"""
    local_key, local_of_key = length_order(seq_index)
    n = len(local_key)
    if len(result) != n:
        raise ValueError("Sequence db size != result db size")
    aln = dict(result)
    if len(aln) != len(result):
        raise ValueError("a key occurs twice in the result DB")
    lists = []
    for i in range(n):
        if local_key[i] not in aln:
            raise ValueError("no entry for key %d in the result DB" % local_key[i])
        data, out = aln[local_key[i]], []
        for line in data.split(b"\n"):
            if not line:
                continue
            word = first_column(line)
            if not word.isdigit() or int(word) not in local_of_key:
                raise ValueError("Element %r contained in some alignment list, but not contained in the sequence database!" % word)
            out.append(local_of_key[int(word)])
        lists.append(out or [i])
    return local_key, lists


def symmetrise(lists):
    """findMissingLinks + addMissingLinks: the lists with every unanswered line appended to the list of the sequence it names, in the order the
    reference appends them (ascending set id, line order).  A line listed twice is taken twice; the reverse is looked for among the lines as read"""
    n = len(lists)
    srt = [sorted(l) for l in lists]
    out = [list(l) for l in lists]
    for s in range(n):
        for e in lists[s]:
            j = bisect.bisect_left(srt[e], s)
            if j == len(srt[e]) or srt[e][j] != s:
                out[e].append(s)
    return out


def visiting_order(sizes):
    """initClustersizes read from the back: (size descending, id descending)"""
    return sorted(range(len(sizes)), key=lambda i: (sizes[i], i), reverse=True)


def connected_component(sym, max_iterations):
    """ClusteringAlgorithms.cpp:83-110 on the symmetric lists -> assigned[] (the representative's id of every id)"""
    n = len(sym)
    assigned = [UINT_MAX] * n
    for rep in visiting_order([len(l) for l in sym]):
        if assigned[rep] != UINT_MAX:
            continue
        assigned[rep] = rep
        queue = deque([(rep, 0)])
        while queue:
            cur, cutoff = queue.popleft()
            assigned[cur] = rep
            for e in sym[cur]:
                if assigned[e] == UINT_MAX and cutoff < max_iterations:
                    queue.append((e, cutoff + 1))
                assigned[e] = rep
    return assigned


def order_free(sym, max_iterations):
    """the rule the GPU computes: the components, each under its first member in visiting order -> (assigned[], holds) where `holds` says that
    no node lies deeper than max_iterations + 1 below its representative (where it does not, the GPU refuses)"""
    n = len(sym)
    assigned, depth, holds = [UINT_MAX] * n, [0] * n, True
    for rep in visiting_order([len(l) for l in sym]):
        if assigned[rep] != UINT_MAX:
            continue
        assigned[rep] = rep
        queue = deque([rep])
        while queue:
            cur = queue.popleft()
            for e in sym[cur]:
                if assigned[e] == UINT_MAX:
                    assigned[e] = rep; depth[e] = depth[cur] + 1
                    holds = holds and depth[e] <= max_iterations + 1
                    queue.append(e)
    return assigned, holds


def pairs_of(local_key, assigned):
    return sorted((local_key[assigned[i]], local_key[i]) for i in range(len(assigned)))


def parse_max_iterations(flags):
    w = flags.split()
    return int(w[w.index("--max-iterations") + 1]) if "--max-iterations" in w else 1000      # Parameters.cpp:2171


def clust(seqdb_path, result_path, max_iterations=1000):
    """the cluster DB of a sequence DB and a result DB on disk: [(key, entry bytes)]"""
    result, _ = read_db(result_path)
    local_key, lists = read_lists(read_index(seqdb_path), result)
    return cluster_entries(pairs_of(local_key, connected_component(symmetrise(lists), max_iterations)))


def condition_holds(seqdb_path, result_path, max_iterations=1000):
    result, _ = read_db(result_path)
    return order_free(symmetrise(read_lists(read_index(seqdb_path), result)[1]), max_iterations)[1]


def extract_fixtures(root):
    """cc.tar.gz names the DBs of local.tar.gz and subst.tar.gz as the inputs of its linclust runs: all three are unpacked side by side under `root`"""
    import tarfile
    golden = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
    for name in ("local.tar.gz", "subst.tar.gz", "cc.tar.gz"):
        with tarfile.open(os.path.join(golden, name)) as t:
            t.extractall(root)
    return str(root)


def runs(root):
    """RUNS of cc.tar.gz: [(name, sequence DB, result DB, flags, 'ok' | 'fail')] (fail: the reference ended with an error and wrote no DB)"""
    return [tuple(l.rstrip("\n").split("\t")) for l in open(os.path.join(root, "cc", "RUNS"))]
