"""The lineage table (taxor_lineage_*, taxor_amd/csrc/lineage.h) through the library against the Python restatement in
tests/lca_expect.py: species of a user bin, fields, node numbering, names and ranks, compacted paths, ROOT, and every refusal."""
import pytest

from taxor_amd import _lib
from taxor_amd.search import Lineage
from tests import lca_expect as le


def sp(ub, ids, names, acc=None):
    return dict(organism_name=f"Organism {ub}", accession_id=acc or f"GCF_{ub:09d}.1", taxid=(ids.split(";") or ["0"])[-1] or "0", taxnames_string=names,
                taxid_string=ids, user_bin=ub, seq_len=1000 + ub)


def same(species, n_bins):
    """library == restatement; returns both"""
    got, want = Lineage(species, n_bins), le.Lineage(species, n_bins)
    assert got.n_user_bins == n_bins and got.n_nodes == len(want.ids)
    assert got.ids == want.ids
    assert got.names == [want.name[x] for x in want.ids]
    assert got.ranks == [want.rank[x] for x in want.ids]
    assert [int(p) for p in got.parent] == [want.number[want.parent[x]] if want.parent[x] else _lib.LCA_ROOT for x in want.ids]
    assert [int(d) for d in got.depth] == [want.depth(x) for x in want.ids]
    assert [int(x) for x in got.bin_species] == want.bin_species
    for b in range(n_bins):
        assert got.path_of(b) == [want.number[x] for x in want.paths[b]], b
    assert got.max_depth == max([len(p) for p in want.paths] + [0])
    return got, want


SEVEN = "k__Bacteria;p__Proteobacteria;c__Gammaproteobacteria;o__Enterobacterales;f__Enterobacteriaceae;g__Escherichia;s__Escherichia coli"


def test_paths_of_1_7_and_64_nodes_and_empty_fields():
    deep_ids = ";".join(str(5000 + i) for i in range(64))
    deep_names = ";".join(f"x__N{i}" for i in range(64))
    species = [sp(0, "77", "s__Lonely"),
               sp(1, "2;1224;1236;91347;543;561;562", SEVEN),
               sp(2, deep_ids, deep_names),
               sp(3, "2;;9236;;9543;9561;83333", "k__Bacteria;p__;c__Gammaproteobacteria;;f__Enterobacteriaceae;g__Escherichia;s__Escherichia coli K-12"),   # empty in the middle
               sp(4, ";;1239;91061", "k__;p__;c__Firmicutes;o__Bacilli"),                                                    # empty at the front
               sp(5, "", ""),                                                                                                  # the empty path
               sp(6, ";;", ";;")]
    got, want = same(species, 7)
    assert len(got.path_of(0)) == 1 and len(got.path_of(1)) == 7 and len(got.path_of(2)) == 64 and got.max_depth == 64
    assert got.path_of(5) == [] and got.path_of(6) == []
    assert want.paths[3] == ["2", "9236", "9543", "9561", "83333"] and want.name["9236"] == "Gammaproteobacteria"
    assert want.paths[4] == ["1239", "91061"] and want.parent["1239"] == ""


def test_an_id_with_two_parents_is_refused_by_its_message():
    species = [sp(0, "2;1224;1236", "k__B;p__P;c__G", "ACC_A"), sp(1, "2;;1236", "k__B;p__;c__G", "ACC_B")]
    with pytest.raises(le.Refused):
        le.Lineage(species, 2)
    with pytest.raises(_lib.TaxorError) as ei:
        Lineage(species, 2)
    m = str(ei.value)
    assert ei.value.code == -1 and "id 1236 has two parents" in m and "1224" in m and " 2 " in m and "ACC_A" in m and "ACC_B" in m


def test_65_nodes_are_refused():
    ids = ";".join(str(5000 + i) for i in range(65))
    names = ";".join(f"x__N{i}" for i in range(65))
    with pytest.raises(le.Refused):
        le.Lineage([sp(0, ids, names, "ACC_DEEP")], 1)
    with pytest.raises(_lib.TaxorError) as ei:
        Lineage([sp(0, ids, names, "ACC_DEEP")], 1)
    assert "more than 64 ids" in str(ei.value) and "ACC_DEEP" in str(ei.value) and "5064" in str(ei.value)
    # 64 ids behind a leading "1": the leading id counts
    with pytest.raises(_lib.TaxorError):
        Lineage([sp(0, "1;" + ";".join(str(5000 + i) for i in range(64)), "x__root;" + ";".join(f"x__N{i}" for i in range(64)))], 1)
    with pytest.raises(le.Refused):
        le.Lineage([sp(0, "1;" + ";".join(str(5000 + i) for i in range(64)), "x__root;" + ";".join(f"x__N{i}" for i in range(64)))], 1)


def test_an_id_twice_in_one_path_is_refused():
    species = [sp(0, "2;1224;2", "k__B;p__P;c__B", "ACC_TWICE")]
    with pytest.raises(le.Refused):
        le.Lineage(species, 1)
    with pytest.raises(_lib.TaxorError) as ei:
        Lineage(species, 1)
    assert "id 2 occurs twice" in str(ei.value) and "ACC_TWICE" in str(ei.value)
    species = [sp(0, "2;1;1224", "k__B;x__root;p__P", "ACC_ROOT")]
    with pytest.raises(le.Refused):
        le.Lineage(species, 1)
    with pytest.raises(_lib.TaxorError) as ei:
        Lineage(species, 1)
    assert "id 1 is the root" in str(ei.value) and "below id 2" in str(ei.value) and "ACC_ROOT" in str(ei.value)


def test_names_shorter_than_ids_are_refused():
    species = [sp(0, "2;1224;1236", "k__B;p__P", "ACC_SHORT")]
    with pytest.raises(le.Refused):
        le.Lineage(species, 1)
    with pytest.raises(_lib.TaxorError) as ei:
        Lineage(species, 1)
    assert "3 ids" in str(ei.value) and "only 2 names" in str(ei.value) and "ACC_SHORT" in str(ei.value) and "2;1224;1236" in str(ei.value)
    same([sp(0, "2;1224", "k__B;p__P;c__more names than ids")], 1)          # the other way round is fine


def test_a_path_starting_with_1_starts_at_root():
    species = [sp(0, "1;2;1224", "x__root;k__Bacteria;p__Proteobacteria"), sp(1, "2;1224;1236", "k__Bacteria;p__Proteobacteria;c__Gamma"), sp(2, "1", "x__root")]
    got, want = same(species, 3)
    assert "1" not in got.ids and got.ids == ["1224", "1236", "2"]
    assert got.path_of(0) == [2, 0] and got.path_of(1) == [2, 0, 1] and got.path_of(2) == []
    assert int(got.parent[2]) == _lib.LCA_ROOT


def test_a_user_bin_without_a_species_falls_back_and_the_first_of_two_wins():
    species = [sp(1, "2;10", "k__B;s__first of bin 1", "ACC_1A"), sp(1, "2;11", "k__B;s__second of bin 1", "ACC_1B"), sp(3, "2;12", "k__B;s__bin 3")]
    got, want = same(species, 4)
    assert [int(x) for x in got.bin_species] == [0, 0, 0, 2]           # bins 0 and 2 have no species: species[0]
    assert "11" not in got.ids                                           # the second species of bin 1 is never looked at
    assert got.path_of(0) == got.path_of(1) == got.path_of(2)


def test_names_shorter_than_3_and_node_numbers_byte_wise():
    species = [sp(0, "9;10;100", "k_;p__Ten;s", "A"), sp(1, "9;10;2", ";p__other name for 10;s__Two", "B"), sp(2, "9;9a", "zz;g__", "C")]
    got, want = same(species, 3)
    assert got.ids == ["10", "100", "2", "9", "9a"]                      # "10" before "9"
    by = dict(zip(got.ids, zip(got.names, got.ranks)))
    assert by["9"] == ("", "k") and by["10"] == ("Ten", "p") and by["100"] == ("", "s") and by["2"] == ("Two", "s") and by["9a"] == ("", "g")
    # an empty name field: rank '-'
    got, _ = same([sp(0, "5;6", ";s__x")], 1)
    assert got.ranks[0] == "-" and got.names[0] == ""


def test_no_species_at_all():
    got, _ = same([], 3)
    assert got.n_nodes == 0 and all(got.path_of(b) == [] for b in range(3))
