"""The prefix tree of the reference's ``decoder/prefixTree.py:28-73``: one node per distinct
spelling prefix of the word list.  The last node of a word is ``isWord`` and carries the word's
LM id, inner nodes are ``isPrefix`` (a node may be both); "specials" are single-symbol words
that hang off the root.  ``flatten`` turns the tree into the arrays the device search reads."""
import numpy as np


class Node(object):
    __slots__ = ("isPrefix", "isWord", "children", "id")

    def __init__(self):
        self.isPrefix = False
        self.isWord = False
        self.children = None
        self.id = -1


class _Children(dict):
    """a missing symbol answers with a node that is neither word nor prefix, and is not kept"""

    def __missing__(self, key):
        return Node()


class PrefixTree(object):
    def __init__(self, chars, words, lm, specials=(), space="[space]"):
        """chars: {token: symbol id}; words: iterable of words spelled in single-character
        tokens; lm: anything with ``get_word_id``; specials: tokens that are whole words;
        space: the separator token or its symbol id"""
        self.chars = chars
        self.lm = lm
        self.space = int(chars[space]) if isinstance(space, str) else int(space)
        self.path_count = 0
        self.root = Node()
        self.root.isPrefix = True
        self.root.children = _Children()
        for tok in specials:
            node = self._child(self.root, self._symbol(tok))
            node.isWord = True
            node.id = lm.get_word_id(tok)
        for word in words:
            if not word:
                continue
            node = self.root
            for ch in word:
                node.isPrefix = True
                node = self._child(node, self._symbol(ch))
                self.path_count += 1
            node.isWord = True
            node.id = lm.get_word_id(word)

    def _symbol(self, tok):
        s = int(self.chars[tok])
        if s == self.space or s < 1:
            raise ValueError("PrefixTree: a word cannot contain the symbol %d (%r)" % (s, tok))
        return s

    @staticmethod
    def _child(node, sym):
        if node.children is None:
            node.children = _Children()
        if sym not in node.children:
            dict.__setitem__(node.children, sym, Node())
        return node.children[sym]

    def flatten(self, A):
        """(child int32[nodes, A], word int32[nodes]): breadth-first node numbers with the root 0;
        child[n, c] the node reached from n by symbol c or -1, word[n] the id of the word that
        ends at n or -1"""
        order = [self.root]
        number = {id(self.root): 0}
        i = 0
        while i < len(order):
            node = order[i]
            i += 1
            for sym in sorted(node.children or ()):
                ch = node.children[sym]
                number[id(ch)] = len(order)
                order.append(ch)
        child = np.full((len(order), int(A)), -1, dtype=np.int32)
        word = np.full(len(order), -1, dtype=np.int32)
        for n, node in enumerate(order):
            if node.isWord:
                word[n] = node.id
            for sym, ch in (node.children or {}).items():
                if sym >= A:
                    raise ValueError("PrefixTree.flatten: symbol %d outside an alphabet of %d" % (sym, A))
                child[n, sym] = number[id(ch)]
        return child, word
