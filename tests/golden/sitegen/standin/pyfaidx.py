"""A stand-in for the one corner of pyfaidx that upstream's extractSNPsfromVCF.py touches: Fasta(path)[name][a:b] and
Fasta(path)[name][i], both str()-able, bases as the file has them.  Our own text; used only by make_fixtures.py."""


class Fasta:
    def __init__(self, path):
        self._records = {}
        name = None
        with open(path) as f:
            for line in f:
                line = line.rstrip("\r\n")
                if line.startswith(">"):
                    name = line[1:].split()[0]
                    if name in self._records:
                        raise ValueError("duplicate record %s" % name)
                    self._records[name] = []
                elif line and name is not None:
                    self._records[name].append(line)
        self._records = {n: "".join(parts) for n, parts in self._records.items()}

    def __getitem__(self, name):
        return self._records[name]          # a str: slices and single bases are already str()-able
