"""The refusals of the host's shared BGZF block list (platypus_amd/csrc/host/bgzf_blocks.hpp) with their messages in full, for
tests/test_bgzf_messages_cpu.py (the host twins on the stand-in device) and tests/test_gpu_bgzf_messages.py (the device paths): a source
VCF of three stored blocks of 100, 100 and 79 bytes handed over as one chunk of one fetch (plat_caller_set_source_blocks) and, with the
EOF block behind it, as a whole file (plat_caller_index_bgzf).  The inputs: BSIZE's high byte flipped in block 1 (the block then leaves
its data), an EOF block spliced in front of block 1, an end_coffset one byte past block 1's start, the low CRC32 byte of block 1 flipped.
The strings were taken from the library before the block list existed; the offsets in them are read off the stream's own headers."""
import struct

import numpy as np

from platypus_amd import _lib, synth

TEXT = b"".join(b"20\t%d\t.\tA\tC\t50\tPASS\t.\tGT\t0/1\n" % (1000 + 10 * k) for k in range(9))
DATA = synth.bgzf_stream(TEXT, 100, level=0, eof=False)[0]
AT1 = struct.unpack_from("<H", DATA, 16)[0] + 1                                   # where block 1 starts ...
N1 = struct.unpack_from("<H", DATA, AT1 + 16)[0] + 1                              # ... and its length
SOURCE_ENTRY, INDEX_ENTRY = "plat_caller_set_source_blocks", "plat_caller_index_bgzf"
WHERE = "region 0, file 0, chunk 0"
NO_INFLATE = " cannot be inflated (a bad header, an invalid deflate stream, output other than ISIZE bytes, or a CRC32 mismatch)"


def _flip(data, at, bit):
    return data[:at] + bytes([data[at] ^ bit]) + data[at + 1:]


NO_CHAIN = _flip(DATA, AT1 + 17, 0x80)
EMPTY_IN_FRONT = DATA[:AT1] + synth.BGZF_EOF + DATA[AT1:]
BAD_CRC = _flip(DATA, AT1 + N1 - 8, 1)


def layout_is_as_described():
    assert len(TEXT) == 279 and len(DATA) > AT1 + N1 and struct.unpack_from("<I", DATA, AT1 + N1 - 4)[0] == 100


def source_blocks(data, end_coffset=-1):
    """The argument of NativeCaller.set_source_blocks: one region, one fetch, `data` as its one chunk."""
    return [[(b"20", 0, 1 << 29, [(np.frombuffer(data, dtype=np.uint8), 0, end_coffset, 0)])]]


def source_cases():
    """[(label, set_source_blocks' argument, the message behind the entry point's name)]; every one is PLAT_ERR_BAD_INPUT."""
    return [
        ("the blocks do not chain", source_blocks(NO_CHAIN),
         "the BGZF blocks of " + WHERE + " do not chain: no valid block header at offset %d of its data "
         "(bad magic, no BC subfield, or a block that leaves the data)" % AT1),
        ("an empty block with data behind it", source_blocks(EMPTY_IN_FRONT),
         "block 1 of " + WHERE + " is empty (ISIZE 0) with data behind it: tabix ends a fetch, or cuts a line, there"),
        ("end_coffset off a block boundary", source_blocks(DATA, AT1 + 1),
         "end_coffset %d of " % (AT1 + 1) + WHERE + " is not a block boundary of its data"),
        ("a block that does not inflate", source_blocks(BAD_CRC), "block 1 of " + WHERE + NO_INFLATE),
    ]


def index_cases():
    """[(label, the file's bytes, the message behind the entry point's name)]; every one is PLAT_ERR_BAD_INPUT."""
    return [
        ("the blocks do not chain", NO_CHAIN + synth.BGZF_EOF,
         "the file's BGZF blocks do not chain: no valid block header at offset %d (bad magic, no BC subfield, or a block that leaves the file)" % AT1),
        ("an empty block with data behind it", EMPTY_IN_FRONT + synth.BGZF_EOF, "block 1 is empty (ISIZE 0) with data behind it: tabix ends the file there"),
        ("a block that does not inflate", BAD_CRC + synth.BGZF_EOF, "block 1" + NO_INFLATE),
    ]


def check(nc):
    """Every case refused with PLAT_ERR_BAD_INPUT and exactly its message, and the good stream taken by both entry points afterwards."""
    import pytest
    layout_is_as_described()
    for entry, cases, call in ((SOURCE_ENTRY, source_cases(), nc.set_source_blocks), (INDEX_ENTRY, index_cases(), nc.index_bgzf)):
        for label, arg, message in cases:
            with pytest.raises(_lib.PlatypusDeviceError) as e:
                call(arg)
            assert e.value.code == -9, (entry, label)
            assert str(e.value) == str(_lib.PlatypusDeviceError(-9, entry + ": " + message, entry)), (entry, label)
    nc.set_source_blocks(source_blocks(DATA))
    assert nc.source_blocks_info["n_blocks"] == 3 and nc.source_blocks_info["kept_bytes"] == len(TEXT) and nc.source_blocks_info["lines_kept"] == 9
    nc.set_source_blocks([])
    assert nc.index_bgzf(DATA + synth.BGZF_EOF).endswith(synth.BGZF_EOF)
