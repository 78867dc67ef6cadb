"""What the reference did with each row of tests/golden/proc_kats.json (tests/golden/make_proc_golden.py), as the
record fields of ``pybitmessage_amd.processor`` -- shared by tests/test_proc.py and tests/test_gpu_proc.py."""
from pybitmessage_amd import processor as P

#: the refusing log line's words -> the status that stands for it (src/class_objectProcessor.py:179-258)
LOG_STATUS = [
    ('getpubkey is abnormally long.', P.TOO_LONG),
    ('pubkey request is zero.', P.VERSION_ZERO),
    ('pubkey request is 1 which', P.VERSION_ONE),
    ('pubkey request is too high.', P.VERSION_TOO_HIGH),
    ('The length of the requested hash', P.SHORT_HASH),
    ('The length of the requested tag', P.SHORT_TAG),
    ('This getpubkey request is not for any of my keys.', P.NOT_MINE),
    ('but the requestedAddressVersionNumber', P.VERSION_MISMATCH),
    ('but the stream number', P.STREAM_MISMATCH),
    ('it is for one of my chan addresses.', P.CHAN),
    ('BUT we already sent it recently.', P.SENT_RECENTLY),
]
COMMAND_STATUS = {name: status for status, name in P.COMMANDS.items()}
ROUTES = {P.OBJECT_GETPUBKEY: P.GETPUBKEY, P.OBJECT_PUBKEY: P.PUBKEY, P.OBJECT_MSG: P.MSG, P.OBJECT_BROADCAST: P.BROADCAST,
          P.OBJECT_ONIONPEER: P.ONIONPEER}


def address_table(kats):
    return P.address_rows((a['version'], a['stream'], bytes.fromhex(a['ripe']), a['chan'], a['last'])
                          for a in kats['addresses'])


def objects(kats):
    return [bytes.fromhex(r['data']) for r in kats['rows']], [r['type'] for r in kats['rows']]


def expected_status(row):
    """The status the reference's behaviour stands for; exactly one piece of evidence per row."""
    route = ROUTES.get(row['type'], P.UNKNOWN_TYPE)
    if route not in (P.GETPUBKEY, P.ONIONPEER):
        assert row['command'] is None and row['peer'] is None and row['exception'] is None
        assert (row['log'] is not None) == (route == P.UNKNOWN_TYPE)
        return P.NONE
    if row['exception'] is not None:
        assert row['command'] is None and row['peer'] is None
        return {'varintDecodeError': P.MALFORMED, 'ValueError': P.RAISES}[row['exception']]
    if row['command'] is not None:
        return COMMAND_STATUS[row['command'][0]]
    if route == P.ONIONPEER:
        return P.PEER if row['peer'] is not None else P.NO_HOST
    hits = [status for words, status in LOG_STATUS if words in row['log']]
    assert len(hits) == 1, row['log']
    return hits[0]


def check_verdict(kats, row, rec, data, table):
    """rec (a REC_DTYPE row) against what the reference did with the object, but for the ack fields."""
    name = row['name']
    assert rec['route'] == ROUTES.get(row['type'], P.UNKNOWN_TYPE), name
    want = expected_status(row)
    assert rec['status'] == want, (name, int(rec['status']), want)
    key = data[int(rec['key_off']):int(rec['key_off']) + int(rec['key_len'])]
    if want in (P.SEND_V2, P.SEND_V3):
        assert key.hex() == row['command'][1] and rec['key_len'] == 20, name
    if want == P.SEND_V4:
        assert kats['addresses'][int(rec['address'])]['address'] == row['command'][1] and rec['key_len'] == 32, name
    if want in (P.SHORT_HASH, P.SHORT_TAG):
        assert rec['key_len'] < (20 if want == P.SHORT_HASH else 32) and rec['key_off'] + rec['key_len'] == len(data), name
    if want in (P.VERSION_MISMATCH, P.STREAM_MISMATCH, P.CHAN, P.SENT_RECENTLY, P.SEND_V2, P.SEND_V3, P.SEND_V4):
        a = table[int(rec['address'])]
        assert key in (a['ripe'].tobytes(), a['tag'].tobytes()), name
    else:
        assert rec['address'] == P.NO_ROW, name
    if want == P.PEER:
        stream, host, port = row['peer']
        assert (int(rec['stream']), int(rec['port'])) == (stream, port), name
        assert P.host_string(data, rec) == host, name
        assert rec['host_off'] + rec['host_len'] == len(data), name
    else:
        assert rec['host_class'] == P.HOST_NONE and rec['host_len'] == 0, name


def expected_acks(kats):
    """Per row ``(ack, ack_aux, ack_first)`` of one sequential run over the fixture's rows: the rows where the
    reference deleted a key are FOUND; a later row with the same tail is FOUND_EARLIER."""
    aux = {bytes.fromhex(k): i for i, k in enumerate(kats['watch'])}
    found, out = {}, []
    for i, row in enumerate(kats['rows']):
        data = bytes.fromhex(row['data'])
        tail = data[16:]
        if len(data) < 32:
            assert not row['ack_left']
            out.append((P.NOT_CHECKED, 0, P.NO_ROW))
        elif row['ack_left']:
            assert tail in aux and tail not in found
            found[tail] = i
            out.append((P.FOUND, aux[tail], i))
        elif tail in found:
            out.append((P.FOUND_EARLIER, aux[tail], found[tail]))
        else:
            assert tail not in aux
            out.append((P.NOT_WATCHED, 0, P.NO_ROW))
    assert sorted(k.hex() for k in aux if k not in found) == kats['watch_left']
    return out
