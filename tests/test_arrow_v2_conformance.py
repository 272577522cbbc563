"""Arrow v2 wire-schema conformance against the REFERENCE SOURCE.

VERDICT.md missing#4/weak#2: round-1 validated our v2 bytes only
against pyarrow and an in-repo fake server built from the same codecs.
A real Parca server cannot run offline, so this test breaks the closed
loop differently: the EXPECTED schema comes from the reference agent's
reporter/arrow_v2.go —

  * field ORDER and the schema-version metadata pair are recorded in
    tests/golden/arrow_v2_reference_schema.json, extracted from
    ArrowSamplesFieldV2's ``fields[N] = <Var>`` assignments, each Var's
    ``Name:`` literal (arrow_v2.go:581-604) and the MetadataSchemaVersion
    constants, so the suite needs no reference checkout to run;
  * field TYPES are transcribed here construct-by-construct with
    file:line citations and compared against the schema pyarrow (an
    independent C++ Arrow implementation) re-parses from our actual
    IPC bytes — names, nesting, dictionary index widths, REE run-end
    types, timestamp unit/tz, UUID extension storage, nullability and
    the schema-version metadata.

What this cannot prove offline: the Go server's manual v2 reader
accepting the bytes end-to-end (BASELINE config 5); that remains
documented as unproven in docs/.
"""

import json
import os

import pyarrow as pa

from parca_agent_amd.model import Frame, FrameType, MappingFile, Trace
from parca_agent_amd.reporter.arrow_v2 import (
    SampleWriterV2,
    serialize_record,
)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                      "golden", "arrow_v2_reference_schema.json")


def _ref_schema():
    with open(GOLDEN) as fh:
        return json.load(fh)


def _emit_batch():
    w = SampleWriterV2()
    m = MappingFile(file_id="c" * 32, path="/usr/bin/app", build_id="bid")
    trace = Trace(frames=(
        Frame(kind=FrameType.NATIVE, address=0x10, mapping=m,
              function_name="f", source_file="a.c", source_line=3),
        Frame(kind=FrameType.KERNEL, address=0x20,
              mapping=MappingFile(path="[kernel.kallsyms]")),
    ))
    w.append_sample(trace, labels={"node": "n1"}, value=1,
                    timestamp_ns=1_700_000_000_000_000_000,
                    sample_type="samples",
                    sample_unit="count", period_type="cpu",
                    period_unit="nanoseconds", temporality="delta",
                    period=52631578, duration_ns=10**9)
    batch = w.build_record()
    # round-trip through IPC bytes: validate what goes on the WIRE,
    # not the in-memory batch.
    data = serialize_record(batch, compress="lz4")
    reader = pa.ipc.open_stream(pa.BufferReader(data))
    out = reader.read_next_batch()
    out_schema = reader.schema
    return out, out_schema


def test_field_order_matches_reference_source():
    expected = _ref_schema()["field_order"]
    assert len(expected) == 13

    _batch, schema = _emit_batch()
    assert schema.names == expected, (schema.names, expected)


def test_types_match_reference_definitions():
    _batch, schema = _emit_batch()

    # Dictionary helper shapes (arrow_v2.go:37-78): uint32 indices over
    # string values.
    str_dict = pa.dictionary(pa.uint32(), pa.string())
    # REE string / numeric columns (arrow_v2.go:115-150, int32 run ends)
    ree_str = pa.run_end_encoded(pa.int32(), pa.string())

    # FunctionFieldTypeV2 (arrow_v2.go:43-48)
    function_struct = pa.struct([
        pa.field("system_name", pa.string_view(), nullable=True),
        pa.field("filename", str_dict, nullable=True),
        pa.field("start_line", pa.uint64(), nullable=False),
    ])
    # LineFieldTypeV2 (arrow_v2.go:56-60)
    line_struct = pa.struct([
        pa.field("line", pa.uint64(), nullable=False),
        pa.field("column", pa.uint64(), nullable=False),
        pa.field("function", pa.dictionary(pa.uint32(), function_struct),
                 nullable=False),
    ])
    # LocationTypeV2 (arrow_v2.go:81-88)
    location_struct = pa.struct([
        pa.field("address", pa.uint64(), nullable=False),
        pa.field("frame_type", str_dict, nullable=True),
        pa.field("mapping_file", str_dict, nullable=True),
        pa.field("mapping_build_id", str_dict, nullable=True),
        pa.field("lines", pa.list_view(line_struct), nullable=True),
    ])
    # StacktraceTypeV2 (arrow_v2.go:97-100)
    stacktrace_type = pa.list_view(
        pa.dictionary(pa.uint32(), location_struct))

    by_name = {f.name: f for f in schema}
    assert by_name["stacktrace"].type.equals(stacktrace_type), \
        by_name["stacktrace"].type
    # StacktraceIDFieldV2: UUID extension == 16-byte fixed storage
    # (arrow_v2.go:149-152)
    st_id = by_name["stacktrace_id"].type
    storage = getattr(st_id, "storage_type", st_id)
    assert storage.equals(pa.binary(16)), st_id
    # ValueField int64 (arrow.go:402-405)
    assert by_name["value"].type.equals(pa.int64())
    # REE string columns (arrow_v2.go:113-146)
    for name in ("producer", "sample_type", "sample_unit", "period_type",
                 "period_unit", "temporality"):
        assert by_name[name].type.equals(ree_str), (name, by_name[name])
    # PeriodField: REE<int32, int64> (arrow.go:455-458)
    assert by_name["period"].type.equals(
        pa.run_end_encoded(pa.int32(), pa.int64()))
    # DurationFieldV2: REE<int32, uint64> (arrow_v2.go:143-146)
    assert by_name["duration"].type.equals(
        pa.run_end_encoded(pa.int32(), pa.uint64()))
    # TimestampFieldV2: ns, UTC (arrow_v2.go:108-111)
    assert by_name["timestamp"].type.equals(
        pa.timestamp("ns", tz="UTC"))
    # labels: struct of per-label REE dict columns (arrow_v2.go:154-161)
    labels_t = by_name["labels"].type
    assert pa.types.is_struct(labels_t)
    node_f = labels_t.field("node")
    assert node_f.type.equals(
        pa.run_end_encoded(pa.int32(), str_dict)), node_f.type


def test_metadata_key_value_from_reference():
    ref = _ref_schema()
    key, val = ref["metadata_key"], ref["metadata_value"]
    _batch, schema = _emit_batch()
    assert schema.metadata[key.encode()] == val.encode()


def test_listview_offsets_valid_after_wire_roundtrip():
    batch, _schema = _emit_batch()
    batch.validate(full=True)  # arrow C++ deep validation on wire bytes
    st = batch.column(batch.schema.get_field_index("stacktrace"))
    assert st.offsets[0].as_py() is not None
