"""Plain, sequential Python restatement of the reference's `clust --cluster-mode 2 | 3` (greedy incremental clustering, the low-memory
variant) and of what linclust's createsubdb + filterdb leave of a prefilter DB: what plasship_clust_greedy_* and plasship_cands_filter have
to compute.  It stands where the CPU oracle stands for the other modules and is itself pinned byte for byte to the reference's DBs in
tests/golden/clust.tar.gz (tests/test_clust_host.py).  The loops run in the reference's order, one element after the other, the correction
pass in place: the parallel form the GPU uses is argued in plass_amd/csrc/clust.hip, not assumed here.

Restated (lib/mmseqs/src): commons/DBReader.cpp:298-315 with DBReader.h:367-379 (SORT_BY_LENGTH), clustering/ClusteringAlgorithms.cpp:17-23,
38-47,127-145,271-332 (execute, greedyIncrementalLowMem), clustering/Clustering.cpp:32-114 (run, writeData), util/createsubdb.cpp and
util/filterdb.cpp:85-178,389-410 as lib/mmseqs/data/workflow/linclust.sh:39-56 calls them."""
import os

UINT_MAX = 0xFFFFFFFF


def read_db(path):
    """(list of (key, entry bytes without the trailing NUL) in index order, dbtype)"""
    data = open(path, "rb").read()
    ent = []
    for line in open(path + ".index", "rb"):
        k, o, l = (int(x) for x in line.split()[:3])
        ent.append((k, data[o:o + l - 1]))
    dbtype = int.from_bytes(open(path + ".dbtype", "rb").read(4), "little") & 0x3FFFFFFF
    return ent, dbtype


def read_index(path):
    """[(key, length column)] of <path>.index in file order"""
    return [tuple(int(x) for x in line.split()[:3])[::2] for line in open(path + ".index", "rb")]


def first_column(line):
    """Util::parseKey: the bytes before the first white space"""
    for i, ch in enumerate(line):
        if ch in b" \t\n":
            return line[:i]
    return line


def greedy_low_mem(seq_index, result):
    """seq_index: [(key, length column)] of the sequence DB; result: [(key, entry bytes)] of the result DB (any line format whose first column
    is a key) -> [(representative key, member key)] sorted"""
    seq = sorted(seq_index)                                   # the reader keeps its index in key order; an id is a position in it
    n = len(seq)
    if len(result) != n:
        raise ValueError("Sequence db size != result db size")
    # SORT_BY_LENGTH: ids ordered by length descending, ties by id ascending; local = position in that order
    order = sorted(range(n), key=lambda i: (-seq[i][1], i))
    local_key = [seq[i][0] for i in order]                    # getDbKey(local)
    local_of_key = {k: j for j, k in enumerate(local_key)}    # getId(key)
    aln = dict(result)
    if len(aln) != len(result):
        raise ValueError("a key occurs twice in the result DB")
    assigned = [UINT_MAX] * n
    for i in range(n):
        cluster_key = local_key[i]
        cluster_id = local_of_key[cluster_key]
        if assigned[cluster_id] > cluster_id:
            assigned[cluster_id] = cluster_id
        if cluster_key not in aln:
            raise ValueError("no entry for key %d in the result DB" % cluster_key)
        data = aln[cluster_key]
        pos = 0
        while pos < len(data) and data[pos] != 0:
            end = data.find(b"\n", pos)
            end = len(data) if end < 0 else end
            word = first_column(data[pos:end])
            if not word.isdigit():
                raise ValueError("line of key %d does not start with a key: %r" % (cluster_key, data[pos:end]))
            key = int(word)
            if key not in local_of_key:
                raise ValueError("Element %d contained in some alignment list, but not contained in the sequence database!" % key)
            curr = local_of_key[key]
            if assigned[curr] > cluster_id:
                assigned[curr] = cluster_id
            pos = end + 1
    # correct edges that are not assigned properly: in place, ascending
    for i in range(n):
        a = assigned[i]
        if assigned[a] != a:
            assigned[a] = a
    return sorted((local_key[assigned[i]], local_key[i]) for i in range(n))


def cluster_entries(pairs):
    """Clustering::writeData: [(representative key, entry bytes without the trailing NUL)] in the order written"""
    out, prev, text = [], None, b""
    for rep, member in pairs:
        if rep != prev:
            if prev is not None:
                out.append((prev, text))
            text = b"%d\n" % rep
        if member != rep:
            text += b"%d\n" % member
        prev = rep
    if prev is not None:
        out.append((prev, text))
    return out


def cluster_db_files(entries):
    """(data file, index file) as one writer thread leaves them"""
    data, index, off = b"", b"", 0
    for key, text in entries:
        e = text + b"\0"
        data += e; index += b"%d\t%d\t%d\n" % (key, off, len(e)); off += len(e)
    return data, index


def clust(seqdb_path, result_path):
    """the cluster DB of a sequence DB and a result DB on disk: [(key, entry bytes)]"""
    result, _ = read_db(result_path)
    return cluster_entries(greedy_low_mem(read_index(seqdb_path), result))


def subset_rule(pref, rep_keys):
    """linclust.sh:39-56: createsubdb --subdb-mode 1 with the cluster DB's keys, then filterdb --filter-file with the same list (a positive
    filter on the first column, compared as strings): [(key, entry bytes)] of pref_filter2, in the list's order"""
    names = {b"%d" % k for k in rep_keys}
    ent = dict(pref)
    out = []
    for k in rep_keys:
        if k not in ent:
            raise ValueError("representative %d has no entry in the prefilter DB" % k)
        kept = b""
        for line in ent[k].split(b"\n"):
            if line and first_column(line) in names:
                kept += line + b"\n"
        out.append((k, kept))
    return out


def parse_cluster_mode(flags):
    w = flags.split()
    return int(w[w.index("--cluster-mode") + 1]) if "--cluster-mode" in w else 0


def extract_fixtures(root):
    """clust.tar.gz names the DBs of hamming.tar.gz as its inputs: both are unpacked side by side under `root`"""
    import tarfile
    golden = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
    for name in ("hamming.tar.gz", "clust.tar.gz"):
        with tarfile.open(os.path.join(golden, name)) as t:
            t.extractall(root)
    return str(root)
